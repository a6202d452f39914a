"""Frame mosaics of the pooled Winograd launches and the 6x6 mosaic of the 52x52 layers (csrc/winograd.hip: vpixel / pooled_pixel,
csrc/network.hip: wino_geometry).

A launch's frame pitch is H + 1 / W + 1, and the next even number where the launch pools: frame origins and tile origins are then even,
so a 2x2 pooling window never straddles a tile or a frame.  The tests run the F(6x6) form on the split GEMM (fp16 and bf16 terms) through
dt_conv2d at the smallest shapes at which the mosaic is chosen and the indexing can go wrong, against the oracle at the F(6x6) bar of
test_gpu_parity.test_conv2d_winograd_vs_oracle (2e-4 of the output's largest value), and against the same launch without the mosaic at
the slot-dependence bar of DESIGN.md 4.3 (2e-5, relative to the output's largest value like test_detector_batch_invariance_full_size).

Bit for bit: G of F(6x6) holds 2/9, 1/90, ... which are no float32 numbers, so no F(6x6) result is exact.  The exact one-hot check
therefore runs the F(2x2) instance of the same output kernel template (halves and small integers only) on a forced 3x3 mosaic; the
F(6x6) kernels -- lane-cooperative and thread-per-item -- hold the one-hot bar of test_conv2d_winograd_detects_transpose (integers
up to 250, off by >= 1 wherever a tap, a separator or a pooling window is misplaced).  Each transform TAKEN ALONE is exact on small
integers (Bt and At are dyadic): tests/test_gpu_wino_transform.py holds every transform kernel, F(6x6) included, to `array_equal`."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from utility import synth
from test_gpu_parity import _detector, dev, relerr

F6_TOL = 2e-4        # test_conv2d_winograd_vs_oracle, F(6x6)
SLOT_TOL = 2e-5      # a frame's bits depend on its slot in its group at rounding level

FORMS = {"f16x2": {}, "bf16x3": {"DT_S3_H2": "0"}}


# ---- the geometry rule, restated (network.hip:wino_geometry) -----------------------------------------------------------------------
def geometry(ts, B, H, W, pooled, force=-1):
    """-> (g, tiles per frame of whole groups)"""
    ph, pw = ((H + 2) & ~1, (W + 2) & ~1) if pooled else (H + 1, W + 1)
    g_best, best = 1, float(-(-H // ts) * -(-W // ts))
    for g in range(2, 7):
        t = float(-(-g * ph // ts) * -(-g * pw // ts)) / (g * g)
        if force != 1 and ((t < best * 0.97 and B >= g * g) or force == g):
            g_best, best = g, t
    return g_best, best


@pytest.mark.parametrize("ts,B,H,W,pooled,g,tiles", [
    (6, 1440, 26, 26, True, 3, 21.78),      # conv_13: pitch 28, 84 = 14 tiles
    (6, 1440, 52, 52, False, 6, 78.03),     # conv_6: pitch 53, 318 = 53 tiles
    (6, 1440, 13, 13, False, 3, 5.44),      # the 13x13 layers stay
    (6, 1440, 26, 26, False, 2, 20.25),     # conv_9 / conv_11 stay
    (4, 48, 13, 13, False, 2, 12.25),       # the recurrent step stays
    (6, 1440, 52, 52, True, 1, 81.0),       # conv_8: pitch 54 = 9 tiles for every g
    (6, 9, 8, 8, True, 3, 2.78),            # the shapes of the GPU cases below
    (6, 11, 8, 14, True, 3, 4.44),
    (6, 9, 26, 26, True, 3, 21.78),
    (6, 36, 52, 52, False, 6, 78.03),
    (6, 37, 52, 52, False, 6, 78.03),
    (6, 35, 52, 52, False, 1, 81.0),        # fewer frames than one group
    (6, 8, 26, 26, True, 1, 25.0),
])
def test_geometry_rule(ts, B, H, W, pooled, g, tiles):
    got_g, got_t = geometry(ts, B, H, W, pooled)
    assert got_g == g and abs(got_t - tiles) < 0.005, (got_g, got_t)
    assert geometry(ts, B, H, W, pooled, force=1)[0] == 1


# ---- layers through dt_conv2d ---------------------------------------------------------------------------------------------------
CASES = {      # B, H, W, Cin, Cout, pool
    "8x8": (9, 8, 8, 32, 128, 1),               # pitch 10, g = 3: 5 tiles exactly
    "8x8_both": (9, 8, 8, 32, 128, 2),
    "ragged_group": (11, 8, 14, 32, 128, 1),    # last group 2 of 9 frames, pitches 10 / 16
    "ragged_group_both": (11, 8, 14, 32, 128, 2),
    "conv_13": (9, 26, 26, 32, 128, 2),         # conv_13's own geometry and epilogue
    "conv_13_pool": (9, 26, 26, 32, 128, 1),
    "thread_per_item": (38, 26, 26, 32, 512, 2),    # 980 tiles x 256 channel pairs: wino_output_kernel<6,2> instead of the lane-cooperative kernel
    "52x52_36": (36, 52, 52, 32, 128, 0),       # one whole 6x6 group
    "52x52_37": (37, 52, 52, 32, 128, 0),       # ... and a group of one frame
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """seeded inputs and the oracle's conv + LeakyReLU (+ 2x2 max), computed once per case"""
    B, H, W, Cin, Cout, pool = CASES[name]
    rs = np.random.RandomState(sum(CASES[name]))
    x = rs.randn(B, H, W, Cin).astype(np.float32)
    w = (rs.randn(3, 3, Cin, Cout) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = rs.randn(Cout).astype(np.float32)
    ref = orc.conv2d(x, w, b)
    ref = np.where(ref > 0, ref, ref * np.float32(0.1)).astype(np.float32)
    refs = {0: [ref], 1: [orc.maxpool2(ref)], 2: [ref, orc.maxpool2(ref)]}[pool]
    for a in refs:      # shared among the cases of a test: left unchanged
        a.setflags(write=False)
    return x, w, b, refs


def _f6_split(monkeypatch, form):
    monkeypatch.setenv("DT_WINO", "2")
    monkeypatch.setenv("DT_WINO_TILE", "6")
    monkeypatch.setenv("DT_S3", "2")
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)


def _run(ctx, x, w, b, pool, slope=0.1):
    ctx.profile_reset(); ctx.profile_enable(True)
    got = ctx.conv2d(dev(x, ctx), w, b, leaky_slope=slope, pool=pool)
    ctx.profile_enable(False)
    names = {n for n in ctx.profile_names() if ctx.profile_read(n)["launches"]}
    return [g.cpu().numpy() for g in (got if pool == 2 else (got,))], names


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["8x8", "8x8_both", "ragged_group", "ragged_group_both", "conv_13", "conv_13_pool", "52x52_36", "52x52_37"])
def test_mosaic_layer_vs_oracle_and_no_mosaic(ctx, monkeypatch, name, form):
    B, H, W, Cin, Cout, pool = CASES[name]
    x, w, b, refs = _case(name)
    _f6_split(monkeypatch, form)
    want = "wino_mosaic:g%d_ts6" % (3 if pool else 6)
    assert geometry(6, B, H, W, pool != 0)[0] == (3 if pool else 6)
    outs, names = _run(ctx, x, w, b, pool)
    assert want in names and "s3_form:" + form in names and "conv_gemm_s3" in names, sorted(names)
    monkeypatch.setenv("DT_WINO_MOSAIC", "1")
    plain, names1 = _run(ctx, x, w, b, pool)
    assert "wino_mosaic:g1_ts6" in names1 and want not in names1 and "s3_form:" + form in names1, sorted(names1)
    for a, p, r in zip(outs, plain, refs):
        e, e1, d = relerr(a, r), relerr(p, r), relerr(a, p)
        print("%s %s: mosaic vs oracle %.3g, no mosaic vs oracle %.3g, mosaic vs no mosaic %.3g" % (name, form, e, e1, d))
        assert a.shape == r.shape and e < F6_TOL and e1 < F6_TOL, (e, e1)
        assert d < SLOT_TOL, d


@pytest.mark.gpu
def test_mosaic_pool_both_thread_per_item_kernel(ctx, monkeypatch):
    """enough (tile, channel pair) items that the launch leaves the lane-cooperative kernel: the pooled branch of wino_output_kernel<6,2>"""
    B, H, W, Cin, Cout, pool = CASES["thread_per_item"]
    assert ((B + 8) // 9) * 14 * 14 * (Cout // 2) >= 768 * 256      # winograd.hip: WINO_COOP_MAX_ITEMS
    x, w, b, refs = _case("thread_per_item")
    _f6_split(monkeypatch, "f16x2")
    outs, names = _run(ctx, x, w, b, pool)
    assert "wino_mosaic:g3_ts6" in names and "s3_form:f16x2" in names, sorted(names)
    monkeypatch.setenv("DT_WINO_MOSAIC", "1")
    plain, names1 = _run(ctx, x, w, b, pool)
    assert "wino_mosaic:g1_ts6" in names1, sorted(names1)
    for a, p, r in zip(outs, plain, refs):
        e, e1, d = relerr(a, r), relerr(p, r), relerr(a, p)
        print("thread_per_item: mosaic vs oracle %.3g, no mosaic vs oracle %.3g, mosaic vs no mosaic %.3g" % (e, e1, d))
        assert a.shape == r.shape and e < F6_TOL and e1 < F6_TOL, (e, e1)
        assert d < SLOT_TOL, d


# ---- one-hot weights --------------------------------------------------------------------------------------------------------------
def _one_hot(B, H, W, Cin, Cout):
    x = (np.arange(B * H * W * Cin, dtype=np.float32).reshape(B, H, W, Cin) * 7 % 251)
    w = np.zeros((3, 3, Cin, Cout), dtype=np.float32)
    for n in range(Cout):
        w[n % 3, (n // 3) % 3, (n * 7) % Cin, n] = 1.0
    return x, w


def _shifted_pooled(x, w):
    """what a single tap = 1 per output channel computes: the input shifted by the tap ('same' zeros), then 2x2 max -- no arithmetic at all"""
    B, H, W, Cin = x.shape
    Cout = w.shape[3]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    full = np.empty((B, H, W, Cout), dtype=np.float32)
    for n in range(Cout):
        dy, dx, ci = [int(v[0]) for v in np.nonzero(w[:, :, :, n])]
        full[..., n] = xp[:, dy:dy + H, dx:dx + W, ci]
    return full, full.reshape(B, H // 2, 2, W // 2, 2, Cout).max(axis=(2, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("pool", [1, 2], ids=["pool", "both"])
def test_pooled_mosaic_one_hot_bit_exact(ctx, monkeypatch, pool):
    """F(2x2) on a forced 3x3 mosaic, ragged last group, different pitches per axis (10 / 16): every value is a small integer or a
    half of one, so the pooled output IS the shifted, pooled input"""
    monkeypatch.setenv("DT_WINO", "2")
    monkeypatch.setenv("DT_WINO_TILE", "2")
    monkeypatch.setenv("DT_WINO_MOSAIC", "3")
    x, w = _one_hot(11, 8, 14, 32, 96)
    full, pooled = _shifted_pooled(x, w)
    outs, names = _run(ctx, x, w, None, pool, slope=1.0)
    assert "wino_mosaic:g3_ts2" in names and "wino_output" in names, sorted(names)
    assert np.array_equal(outs[-1], pooled)
    if pool == 2:
        assert np.array_equal(outs[0], full)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,H,W,Cout", [("coop6", 11, 8, 14, 128), ("thread_per_item", 40, 8, 14, 2560)])
def test_pooled_mosaic_one_hot_f6(ctx, monkeypatch, name, B, H, W, Cout):
    """the same through both F(6x6) output kernels on the mosaic the rule picks (g = 3): integers up to 250, a misplaced tap, separator
    or pooling window is off by >= 1"""
    assert (((B + 8) // 9) * 5 * 8 * (Cout // 2) >= 768 * 256) == (name == "thread_per_item")
    _f6_split(monkeypatch, "f16x2")
    x, w = _one_hot(B, H, W, 32, Cout)
    full, pooled = _shifted_pooled(x, w)
    outs, names = _run(ctx, x, w, None, 2, slope=1.0)
    assert "wino_mosaic:g3_ts6" in names, sorted(names)
    assert np.abs(outs[0] - full).max() < 0.05 and np.abs(outs[1] - pooled).max() < 0.05


# ---- the pooled max-|x| publication ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pooled_amax_slot_under_mosaic(monkeypatch):
    """conv_13 of a 12-frame forward (26x26, pooled + skip tensor, 3x3 mosaic with a ragged group) publishes max |x| of its POOLED
    output into slot 13: equal to the maximum of the tensor, with and without the mosaic"""
    monkeypatch.delenv("DT_WINO_MOSAIC", raising=False)
    det, _, _ = _detector(None, 416, 416, 12)
    c = det.model.ctx
    frames = dev(synth.synth_clip(12, 416, 416, 3, seed=6), c)
    outs = {}
    for mos in ("", "1"):
        if mos:
            monkeypatch.setenv("DT_WINO_MOSAIC", mos)
        c.reload_policy()
        c.profile_reset(); c.profile_enable(True)
        out = c.detector_extract(frames, "max_pooling2d_5")
        c.profile_enable(False)
        assert c.profile_read("wino_output:conv_13")["launches"] == 1
        assert (c.profile_read("wino_mosaic:g3_ts6")["launches"] > 0) == (mos == "")
        a = out.abs().max().item()
        assert a > 0 and np.float32(c.amax_read(13)) == np.float32(a), (mos, c.amax_read(13), a)
        outs[mos] = out
    d = relerr(outs[""].cpu().numpy(), outs["1"].cpu().numpy())
    print("max_pooling2d_5 (conv_1 .. conv_13), mosaic vs no mosaic: %.3g" % d)
    monkeypatch.delenv("DT_WINO_MOSAIC")
    c.reload_policy()
