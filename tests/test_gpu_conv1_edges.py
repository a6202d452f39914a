"""GPU suite: conv_1's direct kernels (csrc/conv1.hip: x/255, 3x3 convolution on RGB, bias, LeakyReLU, 2x2 max) ALONE, through the production
launcher, at the smallest shapes at which each of their mechanisms exists -- against the integer / float64 references of tests/conv1_cases.py, bit
for bit wherever the operands allow it.

The detector-level tests reach these kernels on dense random frames at a relative tolerance, always with one tile per workgroup and always in
the whole-tile uint8 instance.  Here the test entry dt_conv1 (Context.conv1) hands the launcher frames of any size, type and byte alignment and
a forced number of tiles per workgroup, and reports WHICH INSTANCE ran with what walk on what grid (the launcher's own plan_conv1); every case
asserts that against conv1_cases.plan() before it looks at a value, so a moved threshold fails here instead of moving coverage.  The output
buffer is pre-filled with a NaN bit pattern, guard bands in front and behind included: every owned word must be written and every other word
must keep the pattern.  The frames lie between bands of 0xFF bytes (float32: NaN), so a read that should have been zero padding shows in a sum.
Families P / I / Ib / Tp are compared with array_equal and a failure names the tile, workgroup, position in the walk, register set, loop and
lane (conv1_cases.locate), for float32 position codes also the pixel the wrong value came from; T and D are held to t_bar() / d_bar1().

The four instances -> the groups that run them (conv1_cases.py; the CPU suite asserts the table reaches all four, with every walk kind on each):
  full  (uint8, whole tiles)    W, Wb, R, A (offset 0), M, L     production: every detector forward on uint8 frames
  u8    (uint8, guarded)        W, Wb, R, E, M                   production: never (dt_detector_config demands multiples of 32)
  f32   (float32 frames)        W, Wb, R, E, E2, M               production: float32 frames
  mfma  (fp32 MFMA kernel)      W, Wb, R (no tables), E2 (W % 4 == 2), A (byte offsets 1..3)      production: DT_S3_CONV1=0, unaligned uint8 views

Findings: none in the kernels -- every case passed on the first run.  That the cases can fail was tried once on a deliberately wrong build (wrong
values only): with the pair loop handing both tiles of a pair the same register set, 23 whole-tile cases failed -- every I / P / D / T case of W
and Wb that walks a pair -- and the end-to-end test; with each form's smallest partial product left out, all 12 split-instance T cases and all 69
float32 position-code cases failed; nothing else did.  The launcher now refuses B > 65535 (the grid's z limit; it used to fail at launch) and a
negative slope (the split instances take the 2x2 max before the activation): test_launcher_refusals.  The detector tags an unaligned uint8 call
conv1_direct:f32 now (it used to book the split form's FLOPs under :bf16 whatever ran): test_unaligned_frames_end_to_end.

Measured on an MI355X (this file, `pytest -s`), error / bar:
  family T  max |got - ref64| / |ref64|, rms in brackets (bar 2^-21 = 4.77e-07; the emulation: 1.5 / 1.9 x 2^-24, any dropped product >= 125 x 2^-24):
    full  1.63e-07 [3.95e-08]    u8  1.44e-07 [3.82e-08]    f32  1.53e-07 [3.45e-08]    mfma on float32 frames  5.93e-08 [2.49e-08]
    mfma with power-of-two weights (Tp): bit-exact, float32(table[b]) 2^e
  family D  max |got - ref64| / (sum |a||w| + |b|), rms in brackets (bar 2^-18 = 3.81e-06):
    full  6.46e-08 [9.99e-09]    u8  1.03e-07 [1.15e-08]    f32  8.52e-08 [1.15e-08]
    mfma on uint8 2.46e-07 [2.47e-08], on float32 frames 2.07e-07 [2.10e-08], as the fallback (W % 4 = 2, byte offsets) 1.72e-07 [2.07e-08]
  end to end, 256 frames of 64 x 64 at byte offset 1: max_pooling2d_1 4.03e-07 from the aligned call (bar 2e-6); netout 4.64e-05 (aligned) and
    5.28e-05 (offset) from the oracle (NET_TOL 3e-4)
  the whole module: 321 tests in 7 s"""
import numpy as np
import pytest
import torch

import conv1_cases as c1
import mi355_dt

pytestmark = pytest.mark.gpu

S32 = np.uint32(c1.SENTINEL32)
GUARD = 4096            # words in front of and behind the output
BAND = 4096             # bytes (float32: words) in front of and behind the frames
DT_ERR_ARG = 1          # include/mi355_dt.h
SLOT_TEST = 57


@pytest.fixture(autouse=True)
def _policy_env(monkeypatch):
    for k in ("DT_PIN", "DT_S3_CONV1", "DT_S3"):
        monkeypatch.delenv(k, raising=False)


class _Out(object):
    """[B,H/2,W/2,32] float32 pre-filled with the sentinel, a guard band on either side"""

    def __init__(self, ctx, B, H, W):
        self.shape = (B, H // 2, W // 2, 32)
        self.n = int(np.prod(self.shape))
        self.t = torch.full((self.n + 2 * GUARD,), int(S32.view(np.int32)), dtype=torch.int32, device=ctx.device)
        self.view = self.t.view(torch.float32)[GUARD:GUARD + self.n].view(self.shape)

    def words(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(np.uint32)

    def untouched(self):
        return bool((self.words() == S32).all())

    def read(self, what):
        w = self.words()
        stray = np.flatnonzero(np.concatenate([w[:GUARD], w[GUARD + self.n:]]) != S32)
        assert stray.size == 0, "%s: %d words of the guard bands were written (first: word %d of the two bands)" % (what, stray.size, stray[0])
        own = w[GUARD:GUARD + self.n]
        missed = np.argwhere((own == S32).reshape(self.shape))
        assert missed.size == 0, "%s: %d owned words were not written (first: frame %d row %d column %d channel %d)" % ((what, len(missed)) + tuple(missed[0]))
        return own.view(np.float32).reshape(self.shape).copy()


def _upload_frames(ctx, frames, align=0):
    """the frames between two bands of 0xFF bytes (float32: NaN); uint8: at a byte address that is `align` modulo 4"""
    n = frames.size
    if frames.dtype == np.uint8:
        buf = torch.full((2 * BAND + n + 8,), 0xFF, dtype=torch.uint8, device=ctx.device)
        start = BAND + (align - (buf.data_ptr() + BAND)) % 4
    else:
        buf = torch.full((2 * BAND + n,), float("nan"), dtype=torch.float32, device=ctx.device)
        start = BAND
    view = buf[start:start + n].view(frames.shape)
    view.copy_(torch.from_numpy(frames).to(ctx.device))
    assert frames.dtype != np.uint8 or view.data_ptr() % 4 == align
    return view


def _run(ctx, k, o=None):
    """runs the case: (operands, output [B,H/2,W/2,32]); the reported plan is asserted first, the published maximum last"""
    o = o or c1.operands(k)
    out = _Out(ctx, k["B"], k["H"], k["W"])
    info = ctx.conv1(_upload_frames(ctx, o["frames"], k["align"]), o["w"], o["bias"], out.view, slope=k["slope"], split=bool(k["split"]), tpw=k["tpw"],
                     publish=k["publish"])
    assert info == k["want"], "%s: ran %r, the case is about %r" % (k["name"], info, k["want"])
    assert info["instance"] == c1.INSTANCE_CODE[k["inst"]]
    got = out.read(k["name"])
    if k["publish"]:
        amax = ctx.amax_read(SLOT_TEST)
        want = np.abs(got).max() if info["fills_amax"] else np.float32(0.0)
        assert amax.view(np.uint32) == np.float32(want).view(np.uint32), "%s: published max |x| %r, the stored tensor's is %r (fills_amax %d)" % (
            k["name"], float(amax), float(want), info["fills_amax"])
    return o, got


def _source_of(o, v):
    """family P on float32 frames: the pixel a code came from"""
    hit = np.argwhere(o["frames"] == np.float32(abs(v)))
    return "frame %d row %d column %d channel %d" % tuple(hit[0]) if len(hit) else "no pixel holds it"


def _assert_equal(k, o, got, want):
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (k["name"], got.shape, want.shape)
    if np.array_equal(got, want):      # (zeros compare equal whatever their sign; no NaN is expected)
        return
    bad = np.argwhere(got != want)
    b, oy, ox, n = (int(v) for v in bad[0])
    src = ""
    if k["fam"] == "P" and k["dtype"] == "f32":
        src = "; got is the code of %s, expected the one of %s" % (_source_of(o, got[b, oy, ox, n]), _source_of(o, want[b, oy, ox, n]))
    pytest.fail("%s: %d of %d values differ; first at frame %d pooled row %d column %d channel %d (tap %d): got %r expected %r%s; computed at %r" % (
        k["name"], len(bad), got.size, b, oy, ox, n, n % 27, float(got[b, oy, ox, n]), float(want[b, oy, ox, n]), src, c1.locate(k, b, oy, ox, n)))


_SEEN = {}      # (family, instance) -> [max, sum of squares, count, bar]


def _note(k, e, bar):
    s = _SEEN.setdefault((k["fam"], k["inst"] + (" on %s%s" % (k["dtype"], ", fallback" if k["split"] else "") if k["inst"] == c1.MFMA else "")), [0.0, 0.0, 0, bar])
    s[0], s[1], s[2] = max(s[0], float(e.max())), s[1] + float((e * e).sum()), s[2] + e.size
    print("%s: family %s max %.3g rms %.3g of bar %.3g" % (k["name"], k["fam"], e.max(), np.sqrt(np.mean(e * e)), bar))


def _check_case(ctx, k):
    o, got = _run(ctx, k)
    fam = k["fam"]
    if fam in ("P", "I", "Ib", "Tp"):
        want = c1.expected_exact(k, o)
        _assert_equal(k, o, got, want)
        if fam == "Ib":      # the premise: a window of padding alone (= the bias) would have been the maximum
            assert np.abs(want).max(axis=(0, 1, 2)).max() < o["bias"].min() and want.min() > 0
        return
    z = c1.preact(o["x"], o["wx"])
    ref = c1.layer64(z, o["bias"], k["slope"])
    g = got.astype(np.float64)
    if fam == "T":
        nz = ref != 0
        assert np.all(g[~nz] == 0), "%s: %d outputs whose window holds padding and non-positive products only are not 0" % (k["name"], int((g[~nz] != 0).sum()))
        e = np.zeros(ref.shape)
        e[nz] = np.abs(g[nz] - ref[nz]) / np.abs(ref[nz])
        bar = c1.t_bar()
    else:
        e = np.abs(g - ref) / c1.cc.maxpool2(c1.preact_abs(o["x"], o["wx"], o["bias"]))
        bar = c1.d_bar1()
    _note(k, e, bar)
    i = tuple(int(v) for v in np.unravel_index(e.argmax(), e.shape))
    assert e.max() <= bar, (k["name"], float(e.max()), bar, float(got[i]), float(ref[i]), c1.locate(k, *i))


def _param(*groups):
    return pytest.mark.parametrize("name", c1.case_ids(*groups))


@_param("W")
def test_walk(ctx, name):
    _check_case(ctx, c1.CASES[name])


@_param("Wb")
def test_bench_size_walk(ctx, name):
    k = c1.CASES[name]
    assert k["want"]["tpw"] in (13, 26) and -(-(k["W"] // 2) // 8) == 26
    _check_case(ctx, k)


@_param("R")
def test_tile_rows(ctx, name):
    _check_case(ctx, c1.CASES[name])


@_param("E", "E2")
def test_partial_tiles(ctx, name):
    _check_case(ctx, c1.CASES[name])


@_param("A")
def test_byte_alignment(ctx, name):
    k = c1.CASES[name]
    if k["align"]:
        assert k["inst"] == c1.MFMA and k["want"]["fills_amax"] == 0
    _check_case(ctx, k)


@_param("M")
def test_published_maximum_ignores_padding_windows(ctx, name):
    k = c1.CASES[name]
    assert k["publish"] and k["want"]["fills_amax"]
    _check_case(ctx, k)


@_param("L")
def test_the_launchers_own_rule(ctx, name):
    """tpw = 0.  The smallest shape at which production walks more than one tile, and the shapes of the detector-level conv_1 test
    (test_gpu_parity.py), whose launches must be what they were: one tile per workgroup of the whole-tile uint8 instance."""
    k = c1.CASES[name]
    assert k["tpw"] == 0 and k["inst"] == c1.FULL
    if (k["B"], k["H"], k["W"]) == c1.RULE_SHAPE:
        assert k["want"]["tpw"] == 2
    else:
        assert (k["B"], k["H"], k["W"]) in c1.PRODUCTION_SHAPES and k["want"]["tpw"] == 1
    _check_case(ctx, k)


def test_launcher_refusals(ctx):
    """DT_ERR_ARG with a message and no launch: the output keeps its sentinel"""
    w, bias = np.zeros((27, 32), np.float32), np.zeros(32, np.float32)
    for B, H, W, over in ((2, 3, 4, {}), (2, 4, 6 + 1, {}), (2, 4, 4, dict(batch=0)), (65536, 2, 2, {}), (2, 4, 4, dict(slope=-0.1)), (2, 4, 4, dict(tpw=27))):
        for dtype in (np.uint8, np.float32):
            frames = _upload_frames(ctx, np.ones((B, H, W, 3), dtype))
            out = _Out(ctx, B, H, W)
            with pytest.raises(mi355_dt.NativeError, match=r"dt_conv1: the launcher refuses") as ei:
                ctx.conv1(frames, w, bias, out.view, **over)
            assert "dt_conv1 failed (%d)" % DT_ERR_ARG in str(ei.value), (B, H, W, over, str(ei.value))
            assert out.untouched(), (B, H, W, over)


def test_unaligned_frames_end_to_end(ctx):
    """The fallback the detector can really meet: uint8 frames that are a view at byte offset 1 of a larger buffer.  conv_1 runs the fp32 MFMA
    kernel (tagged conv1_direct:f32), publishes no maximum, and conv_2 -- in the direct fp16 form at this batch -- measures its input itself.
    The frames are independent in the reference: the oracle runs on three of them."""
    from test_gpu_parity import NET_TOL, _detector, chan_err, dev, flat_c
    from oracle import oracle as orc
    H = W = 64
    B = 256      # 1024 16x16-pixel blocks of conv_2's input: the direct fp16 form's threshold
    det, layers, _ = _detector(ctx, H, W, 12)
    c = det.model.ctx
    frames = np.random.RandomState(11).randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    aligned = dev(frames, c)
    buf = torch.zeros(frames.size + 8, dtype=torch.uint8, device=c.device)
    start = (1 - buf.data_ptr()) % 4
    offset = buf[start:start + frames.size].view(frames.shape)
    offset.copy_(aligned)
    assert aligned.data_ptr() % 4 == 0 and offset.data_ptr() % 4 == 1

    def profiled(x):
        c.profile_reset(); c.profile_enable(True)
        net = c.detect_forward(x)
        c.profile_enable(False)
        return net.cpu().numpy(), {n for n in c.profile_names() if c.profile_read(n)["launches"]}

    net_a, names_a = profiled(aligned)
    net_o, names_o = profiled(offset)
    for names in (names_a, names_o):
        assert "conv_direct_h2:conv_2" in names, sorted(names)
    assert "conv1_direct:bf16" in names_a and "conv1_direct:f32" not in names_a and "absmax:conv_2" not in names_a, sorted(names_a)
    assert "conv1_direct:f32" in names_o and "conv1_direct:bf16" not in names_o and "absmax:conv_2" in names_o, sorted(names_o)
    pool_a = c.detector_extract(aligned, "max_pooling2d_1").cpu().numpy()
    pool_o = c.detector_extract(offset, "max_pooling2d_1").cpu().numpy()
    e = chan_err(pool_o, pool_a)
    print("max_pooling2d_1, byte offset 1 against aligned: chan_err %.3g" % e)
    assert e < 2e-6, e
    pick = [0, B // 2, B - 1]
    ref_net, _, _ = orc.yolov2_forward(orc.normalize_u8(frames[pick]), layers)
    for what, net in (("aligned", net_a), ("offset", net_o)):
        e = chan_err(flat_c(net[pick]), flat_c(ref_net))
        print("netout, %s against the oracle: chan_err %.3g" % (what, e))
        assert e < NET_TOL, (what, e)


def test_zz_measured_errors_summary():
    """prints what the docstring records (runs last in the module; nothing to assert beyond what the cases asserted)"""
    for (fam, inst), (mx, ss, n, bar) in sorted(_SEEN.items()):
        print("family %s  %-22s max %.3g [rms %.3g] of %.3g" % (fam, inst, mx, np.sqrt(ss / max(n, 1)), bar))
        assert mx <= bar
