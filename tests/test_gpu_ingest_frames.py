"""GPU suite (-m gpu): dt_ingest_frames -- NV12 and row-pitched RGB24 frames at per-frame sizes, converted and resized in one call.

Integer arithmetic only, so every comparison is bit for bit (np.array_equal) against the plain restatement tests/ingest_ref.py:
convert (written out from the definition in include/mi355_dt.h), optional channel swap, then the ORACLE's resize on that frame alone.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ingest_ref as ir
import mi355_dt
from mi355_dt import DT_PIX_NV12, DT_PIX_RGB24, DT_PIX_SWAP_RB, FrameDesc, NativeError
from utility import synth
from utility.frames import ingest_frames, nv12_planes

pytestmark = pytest.mark.gpu


def dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def rand_rgb(rs, h, w):
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def rand_nv12(rs, h, w):
    """random full-range bytes: both clamps of the conversion are reached (tests/test_ingest_frames_cpu.py)"""
    return rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w // 2, 2)).astype(np.uint8)


def to_dev(item, ctx, pitch=None, fill=0xFF):
    """a host item -> the device item; with a pitch the rows lie `pitch` bytes apart in a larger allocation full of `fill`"""
    if isinstance(item, tuple):
        y, uv = item
        if pitch is None:
            return dev(y, ctx), dev(uv, ctx)
        H, W = y.shape
        ys = np.full((H, pitch), fill, dtype=np.uint8)
        ys[:, :W] = y
        us = np.full((H // 2, pitch), fill, dtype=np.uint8)
        us[:, :W] = uv.reshape(H // 2, W)
        dy, du = dev(ys, ctx), dev(us, ctx)                 # two allocations
        return dy[:, :W], du.reshape(-1).as_strided((H // 2, W // 2, 2), (pitch, 2, 1))
    if pitch is None:
        return dev(item, ctx)
    H, W, _ = item.shape
    big = np.full((H, pitch, 3), fill, dtype=np.uint8)
    big[:, :W] = item
    return dev(big, ctx)[:, :W]


def check_frames(got, items, out_h, out_w, swap_rb=False, what=""):
    got = got.cpu().numpy()
    assert got.shape == (len(items), out_h, out_w, 3) and got.dtype == np.uint8
    ref = ir.ingest_frames_ref(items, out_h, out_w, swap_rb)
    for i in range(len(items)):
        if not np.array_equal(got[i], ref[i]):
            bad = np.argwhere(got[i] != ref[i])
            shape = items[i][0].shape if isinstance(items[i], tuple) else items[i].shape
            raise AssertionError("%s frame %d (%s, source %s): %d bytes differ, first at %s: got %d, restatement %d"
                                 % (what, i, "NV12" if isinstance(items[i], tuple) else "RGB24", shape, len(bad), bad[0].tolist(),
                                    got[i][tuple(bad[0])], ref[i][tuple(bad[0])]))


# ------------------------------------------------------------------ 1. against the existing entry
@pytest.mark.parametrize("swap_rb", [False, True], ids=["as_is", "swap_rb"])
def test_tight_rgb24_equals_ingest_resize(ctx, swap_rb):
    rs = np.random.RandomState(1)
    frames = dev(rs.randint(0, 256, (3, 37, 53, 3)).astype(np.uint8), ctx)
    old = ctx.ingest_resize(frames, 64, 64).cpu().numpy()
    got = ctx.ingest_frames([frames[i] for i in range(3)], 64, 64, swap_rb=swap_rb).cpu().numpy()
    assert np.array_equal(got, old[..., ::-1] if swap_rb else old)
    assert len(np.unique(old)) > 100


# ------------------------------------------------------------------ 2. mixed sizes and pitches, RGB24
def test_mixed_sizes_and_pitches_rgb24(ctx):
    """37x53, 64x64 (identity), 20x30 (upscale), 1x1, 3x7, and 130x98 as a view of a 130x128x3 tensor whose bytes beyond column 98 are
    0xFF: a read past the width would pull 0xFF into the last columns.  1x1, 3x7 and the upscale take the `s < 0` and `s >= src - 1`
    branches of the coefficient code."""
    rs = np.random.RandomState(2)
    items = [rand_rgb(rs, h, w) for h, w in ((37, 53), (64, 64), (20, 30), (1, 1), (3, 7))]
    wide = rs.randint(0, 128, (130, 98, 3)).astype(np.uint8)       # below 0x80: 0xFF from beyond the width would stand out
    items.append(wide)
    d_items = [to_dev(a, ctx) for a in items[:-1]] + [to_dev(wide, ctx, pitch=128)]
    assert tuple(d_items[-1].stride()) == (128 * 3, 3, 1) and not d_items[-1].is_contiguous()
    got = ctx.ingest_frames(d_items, 64, 64)
    check_frames(got, items, 64, 64, what="mixed RGB24")
    assert np.array_equal(got[1].cpu().numpy(), items[1]), "64x64 -> 64x64 is the identity"
    assert int(got[5].max()) < 128
    assert np.array_equal(ingest_frames(d_items, 64, 64, ctx=ctx).cpu().numpy(), got.cpu().numpy())      # the module-level helper


# ------------------------------------------------------------------ 3. NV12
@functools.lru_cache(maxsize=None)
def _hd_case():
    """one 1080x1920 decoder-style surface (Y rows, then UV rows, pitch 2048, padding 0xFF) and its restatement at 416x416, computed once"""
    rs = np.random.RandomState(33)
    H, W, P = 1080, 1920, 2048
    surface = np.full((H + H // 2, P), 0xFF, dtype=np.uint8)
    surface[:, :W] = rs.randint(0, 256, (H + H // 2, W))
    item = (np.ascontiguousarray(surface[:H, :W]), np.ascontiguousarray(surface[H:, :W]).reshape(H // 2, W // 2, 2))
    ref = ir.ingest_frames_ref([item], 416, 416)
    ref.setflags(write=False)
    return surface, ref


@pytest.mark.parametrize("swap_rb", [False, True], ids=["as_is", "swap_rb"])
def test_nv12_small(ctx, swap_rb):
    """2x2 (the smallest), 36x52 at pitch 64 with y and uv in separate allocations, 64x64 -> 64x64"""
    rs = np.random.RandomState(3)
    items = [rand_nv12(rs, 2, 2), rand_nv12(rs, 36, 52), rand_nv12(rs, 64, 64)]
    d_items = [to_dev(items[0], ctx), to_dev(items[1], ctx, pitch=64, fill=0x00), to_dev(items[2], ctx)]
    assert tuple(d_items[1][0].stride()) == (64, 1) and tuple(d_items[1][1].stride()) == (64, 2, 1)
    got = ctx.ingest_frames(d_items, 64, 64, swap_rb=swap_rb)
    check_frames(got, items, 64, 64, swap_rb, what="NV12")
    assert np.array_equal(got[2].cpu().numpy(), ir.convert(items[2], swap_rb)), "64x64 -> 64x64 is the conversion alone"


@pytest.mark.parametrize("swap_rb", [False, True], ids=["as_is", "swap_rb"])
def test_nv12_1080p_surface(ctx, swap_rb):
    """1080x1920 -> 416x416 from a single surface through nv12_planes.  The blend works on each channel alone, so the restatement with
    the swap is the cached one with its channels reversed (tests/test_ingest_frames_cpu.py holds the restatement to that)."""
    surface, ref = _hd_case()
    d_surface = dev(surface, ctx)
    y, uv = nv12_planes(d_surface, 1080, 1920, pitch=2048)
    assert y.data_ptr() == d_surface.data_ptr()
    got = ctx.ingest_frames([(y, uv)], 416, 416, swap_rb=swap_rb).cpu().numpy()
    assert np.array_equal(got, ref[..., ::-1] if swap_rb else ref)


# ------------------------------------------------------------------ 4. coefficient bits
# (32, 96), (32, 416), (32, 608): where a CPU sweep found fused and separate rounding of (d + 0.5) * scale - 0.5 to differ
# (tests/test_ingest_frames_cpu.py::test_where_a_contracted_fma_changes_f), beside (1, 5) of the list
COEF_PAIRS = [(1080, 416), (1920, 416), (37, 64), (53, 64), (98, 64), (719, 608), (64, 64), (1, 5), (7, 3), (32, 96), (32, 416), (32, 608)]


@pytest.mark.parametrize("src,dst", COEF_PAIRS, ids=["%d_to_%d" % p for p in COEF_PAIRS])
def test_coefficient_bits(ctx, src, dst):
    """A one-row and a one-column ramp frame (and a random one of each): x0, x1, a0, a1 resp. y0, y1, b0, b1 of every destination index
    show in the output, which equals the oracle's -- whose tables come from the host formula the kernel recomputes."""
    rs = np.random.RandomState(src * 1000 + dst)
    ramp = ((np.arange(src)[:, None] * np.array([1, 3, 7])[None, :] + np.array([0, 85, 170])[None, :]) % 256).astype(np.uint8)
    noise = rs.randint(0, 256, (src, 3)).astype(np.uint8)
    rows = [ramp[None], noise[None]]             # [1, src, 3]
    cols = [ramp[:, None], noise[:, None]]       # [src, 1, 3]
    check_frames(ctx.ingest_frames([to_dev(a, ctx) for a in rows], 1, dst), rows, 1, dst, what="row %d -> %d" % (src, dst))
    check_frames(ctx.ingest_frames([to_dev(a, ctx) for a in cols], dst, 1), cols, dst, 1, what="column %d -> %d" % (src, dst))


# ------------------------------------------------------------------ 5. more frames than one launch carries
def tiny_items(n, seed):
    """formats and sizes alternating by index: 8x8 ... 12x10"""
    rs = np.random.RandomState(seed)
    sizes = [(8, 8), (10, 12), (12, 10), (8, 12), (12, 8)]
    items = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        items.append(rand_nv12(rs, h, w) if i % 2 else rand_rgb(rs, h + (i % 3 == 0), w - (i % 4 == 0)))
    return items


@pytest.mark.parametrize("n", [65, 130])
def test_more_frames_than_one_launch(ctx, n):
    items = tiny_items(n, 50 + n)
    d_items = [to_dev(a, ctx, pitch=16 if i % 5 == 2 else None) for i, a in enumerate(items)]
    check_frames(ctx.ingest_frames(d_items, 32, 32), items, 32, 32, what="n = %d" % n)


# ------------------------------------------------------------------ 6. no per-size state
def test_no_per_size_state(ctx):
    rs = np.random.RandomState(6)
    a_items = [rand_rgb(rs, 37, 53), rand_nv12(rs, 20, 30)]
    b_items = [rand_nv12(rs, 48, 36), rand_rgb(rs, 9, 70), rand_rgb(rs, 64, 64)]
    da, db = [to_dev(a, ctx) for a in a_items], [to_dev(a, ctx) for a in b_items]
    first = ctx.ingest_frames(da, 64, 64).cpu().numpy()
    check_frames(ctx.ingest_frames(db, 48, 80), b_items, 48, 80, what="call B")
    third = ctx.ingest_frames(da, 64, 64).cpu().numpy()
    assert np.array_equal(first, third)
    check_frames(torch.from_numpy(first), a_items, 64, 64, what="call A")


def test_old_entry_keeps_its_table(ctx):
    """ingest_resize(s1), ingest_frames(other sizes), ingest_resize(s1): the new entry touches neither the cached key nor the table"""
    from oracle import oracle as orc
    rs = np.random.RandomState(7)
    src = rs.randint(0, 256, (2, 37, 53, 3)).astype(np.uint8)
    d_src = dev(src, ctx)
    first = ctx.ingest_resize(d_src, 64, 48).cpu().numpy()
    items = [rand_rgb(rs, 90, 21), rand_nv12(rs, 14, 200)]
    check_frames(ctx.ingest_frames([to_dev(a, ctx) for a in items], 64, 48), items, 64, 48, what="between")
    third = ctx.ingest_resize(d_src, 64, 48).cpu().numpy()
    assert np.array_equal(first, third) and np.array_equal(first, orc.resize_bilinear_u8(src, 64, 48))


@pytest.mark.parametrize("n", [3, 65])
def test_launches_per_call(n):
    """ceil(n / 64) launches under the "ingest" name, with the algorithmic bytes of the frames: 1.5 per NV12 source pixel, 3 per RGB24
    source pixel, and the 3 * dst_h * dst_w written per frame (as dt_ingest_resize counts them)"""
    c = mi355_dt.Context()
    try:
        items = tiny_items(n, 8)
        d_items = [to_dev(a, c) for a in items]
        c.profile_reset(); c.profile_enable(True)
        c.ingest_frames(d_items, 32, 32)
        c.profile_enable(False)
        p = c.profile_read("ingest")
        want = sum(1.5 * a[0].size if isinstance(a, tuple) else float(a.size) for a in items) + n * 3.0 * 32 * 32
        assert p["launches"] == (n + 63) // 64, p
        assert p["bytes"] == want, (p, want)
    finally:
        c.close()


# ------------------------------------------------------------------ 7. errors
def _desc(p0, p1, h, w, pitch0, pitch1, fmt, reserved=0):
    return FrameDesc(p0, p1, h, w, pitch0, pitch1, fmt, reserved)


def test_errors_leave_the_destination_untouched(ctx):
    t = torch
    buf = t.zeros(1 << 16, dtype=t.uint8, device=ctx.device)
    P = buf.data_ptr()
    dst = t.full((65, 16, 16, 3), 0xA5, dtype=t.uint8, device=ctx.device)
    D = ctypes.c_void_p(dst.data_ptr())
    good_rgb = _desc(P, None, 8, 8, 24, 0, DT_PIX_RGB24)
    good_nv12 = _desc(P, P + 4096, 8, 8, 8, 8, DT_PIX_NV12 | DT_PIX_SWAP_RB)
    lib, h = ctx.lib, ctx.h
    ctx._sync_stream()

    def call(descs, n=None, d=D, dh=16, dw=16, handle=h, null_desc=False):
        arr = (FrameDesc * max(1, len(descs)))(*descs)
        rc = lib.dt_ingest_frames(handle, None if null_desc else arr, len(descs) if n is None else n, d, dh, dw)
        return rc, lib.dt_last_error(handle).decode()

    assert call([good_rgb, good_nv12])[0] == 0            # the two templates are fine
    dst.fill_(0xA5)
    # whole-call errors
    for kw in (dict(handle=None), dict(null_desc=True), dict(d=None), dict(n=0), dict(n=-1), dict(dh=0), dict(dw=0), dict(dh=-3), dict(dh=65536)):
        rc, _ = call([good_rgb], **kw)
        assert rc == 1, kw                                 # DT_ERR_ARG
    # one bad descriptor, at index 1 of 3
    bad = {
        "null plane0": _desc(None, None, 8, 8, 24, 0, DT_PIX_RGB24),
        "NV12 without plane1": _desc(P, None, 8, 8, 8, 8, DT_PIX_NV12),
        "height 0": _desc(P, None, 0, 8, 24, 0, DT_PIX_RGB24),
        "width 0": _desc(P, None, 8, 0, 24, 0, DT_PIX_RGB24),
        "height -1": _desc(P, None, -1, 8, 24, 0, DT_PIX_RGB24),
        "height 16385": _desc(P, None, 16385, 8, 24, 0, DT_PIX_RGB24),
        "width 16385": _desc(P, None, 8, 16385, 3 * 16385, 0, DT_PIX_RGB24),
        "NV12 odd height": _desc(P, P + 4096, 7, 8, 8, 8, DT_PIX_NV12),
        "NV12 odd width": _desc(P, P + 4096, 8, 7, 8, 8, DT_PIX_NV12),
        "RGB24 pitch0 below 3 * width": _desc(P, None, 8, 8, 23, 0, DT_PIX_RGB24),
        "NV12 pitch0 below width": _desc(P, P + 4096, 8, 8, 7, 8, DT_PIX_NV12),
        "NV12 pitch1 below width": _desc(P, P + 4096, 8, 8, 8, 7, DT_PIX_NV12),
        "unknown format 2": _desc(P, P + 4096, 8, 8, 24, 8, 2),
        "unknown flag 32": _desc(P, None, 8, 8, 24, 0, DT_PIX_RGB24 | 32),
        "negative format": _desc(P, None, 8, 8, 24, 0, -1),
        "reserved 1": _desc(P, None, 8, 8, 24, 0, DT_PIX_RGB24, reserved=1),
    }
    for name, d in sorted(bad.items()):
        rc, msg = call([good_rgb, d, good_nv12])
        assert rc == 1, name
        assert "frame 1" in msg, (name, msg)
    # only the LAST descriptor of a 65-frame call is bad: nothing of the first launch's 64 frames is written either
    rc, msg = call([good_rgb, good_nv12] * 32 + [bad["NV12 odd width"]])
    assert rc == 1 and "frame 64" in msg, msg
    t.cuda.synchronize()
    assert bool((dst == 0xA5).all()), "an error wrote to the destination"
    # the largest accepted size is accepted (one row, so that the frame stays small)
    assert call([_desc(P, None, 1, 16384, 3 * 16384, 0, DT_PIX_RGB24)], dh=1, dw=16)[0] == 0


def test_python_items_are_checked(ctx):
    t = torch
    ok = t.zeros((8, 8, 3), dtype=t.uint8, device=ctx.device)
    y, uv = t.zeros((8, 8), dtype=t.uint8, device=ctx.device), t.zeros((4, 4, 2), dtype=t.uint8, device=ctx.device)
    bad = {
        "float frame": ok.float(),
        "host tensor": ok.cpu(),
        "numpy array": np.zeros((8, 8, 3), dtype=np.uint8),
        "channel-reversed strides": t.zeros((8, 3, 8), dtype=t.uint8, device=ctx.device).permute(0, 2, 1),
        "four channels": t.zeros((8, 8, 4), dtype=t.uint8, device=ctx.device),
        "column-strided": t.zeros((8, 16, 3), dtype=t.uint8, device=ctx.device)[:, ::2],
        "pair of three": (y, uv, uv),
        "pair of one": (y,),
        "uv of another size": (y, t.zeros((4, 3, 2), dtype=t.uint8, device=ctx.device)),
        "host uv": (y, uv.cpu()),
        "planar uv": (y, t.zeros((4, 2, 4), dtype=t.uint8, device=ctx.device).permute(0, 2, 1)),
    }
    for name, item in sorted(bad.items()):
        with pytest.raises(NativeError) as e:
            ctx.ingest_frames([ok, (y, uv), item], 16, 16)
        assert "frame 2" in str(e.value), (name, str(e.value))
    with pytest.raises(NativeError):
        ctx.ingest_frames(ok[None], 16, 16)                # a tensor is not a list of frames
    with pytest.raises(NativeError):
        ctx.ingest_frames([ok], 16, 16, out=t.empty((1, 16, 16, 3), dtype=t.uint8, device=ctx.device)[:, :, ::2])
    # out: a slice of a [streams, T, H, W, 3] batch is filled in place
    batch = t.full((2, 3, 16, 16, 3), 0xA5, dtype=t.uint8, device=ctx.device)
    rs = np.random.RandomState(9)
    items = [rand_rgb(rs, 5, 9), rand_nv12(rs, 6, 4), rand_rgb(rs, 30, 30)]
    ret = ctx.ingest_frames([to_dev(a, ctx) for a in items], 16, 16, out=batch[1])
    assert ret.data_ptr() == batch[1].data_ptr()
    check_frames(batch[1], items, 16, 16, what="out=")
    assert bool((batch[0] == 0xA5).all())


# ------------------------------------------------------------------ 8. fresh versus used context
def test_fresh_and_used_context_agree():
    rs = np.random.RandomState(10)
    items = [rand_nv12(rs, 36, 52), rand_rgb(rs, 21, 17), rand_nv12(rs, 2, 2)]
    big = tiny_items(70, 11) + [rand_nv12(rs, 200, 300), rand_rgb(rs, 150, 90)]

    def target(c):
        return c.ingest_frames([to_dev(a, c, pitch=64) for a in items], 48, 40).cpu().numpy()

    fresh = mi355_dt.Context()
    try:
        want = target(fresh)
    finally:
        fresh.close()
    used = mi355_dt.Context()
    try:
        used.ingest_frames([to_dev(a, used) for a in big], 96, 128)
        used.ingest_resize(dev(rs.randint(0, 256, (4, 50, 60, 3)).astype(np.uint8), used), 48, 40)
        got = target(used)
    finally:
        used.close()
    assert np.array_equal(got, want)
    check_frames(torch.from_numpy(want), items, 48, 40, what="fresh context")


# ------------------------------------------------------------------ 9. plumbing
@pytest.fixture(scope="module")
def small_tracker():
    """96x128 (3x4 grid), C = 12, head scaled so that frames carry boxes (as tests/test_gpu_stream.py builds it); its context is closed
    after the last test here"""
    from models_tracking.MultiObjDetTracker import MultiObjDetTracker

    class Trk(MultiObjDetTracker):
        IMAGE_H, IMAGE_W = 96, 128
        GRID_H, GRID_W = 3, 4
        SEQUENCE_LENGTH = 4
        LOAD_MODEL = False
        OBJ_THRESHOLD = 0.3

    C = len(Trk.LABELS)
    tw = synth.synth_tracker_weights(C)
    tw["out_kernel"] = tw["out_kernel"] * 40.0
    tw["out_bias"][4::5 + C] = 1.5
    trk = Trk(detector_weights=synth.synth_darknet_blob(C), tracker_weights=tw)
    yield trk
    trk.model.ctx.close()


@pytest.mark.parametrize("swap_rb", [False, True], ids=["as_is", "swap_rb"])
def test_detect_on_a_list_of_nv12_frames(monkeypatch, small_tracker, swap_rb):
    det = small_tracker.detector
    monkeypatch.setattr(det, "INGEST_SWAP_RB", swap_rb, raising=False)
    monkeypatch.setattr(det, "OBJ_THRESHOLD", 0.02, raising=False)
    c = det.model.ctx
    rs = np.random.RandomState(12)
    items = [rand_nv12(rs, 120, 160), rand_nv12(rs, 96, 128), rand_nv12(rs, 54, 250)]
    d_items = [to_dev(items[0], c, pitch=192), to_dev(items[1], c), to_dev(items[2], c)]
    tensor = dev(ir.ingest_frames_ref(items, 96, 128, swap_rb), c)
    ref, got = det.detect(tensor), det.detect(d_items)
    for k in ("boxes", "counts"):
        assert torch.equal(got[k], ref[k]), k
    net_ref = det.model.forward(tensor)
    net_got = det.model.forward(c.ingest_frames(d_items, 96, 128, swap_rb=swap_rb))
    assert torch.equal(net_got, net_ref) and bool(torch.isfinite(net_ref).all())
    print("detect: %d boxes" % int(ref["counts"].sum()))


def test_track_stream_on_lists_of_frames(small_tracker):
    """two streams of different source sizes (NV12 at a pitch, RGB24 views), T = 2 per call, two calls: every key of the result equals
    track_stream on the pre-ingested tensor from the same fresh slots"""
    trk = small_tracker
    c = trk.model.ctx
    rs = np.random.RandomState(13)
    s0 = [rand_nv12(rs, 120, 160) for _ in range(4)]
    s1 = [np.ascontiguousarray(f) for f in synth.synth_clip(4, 100, 140, 2, seed=14)]
    d0 = [to_dev(a, c, pitch=192) for a in s0]
    d1 = [to_dev(a, c, pitch=160) for a in s1]
    tensor = dev(np.stack([ir.ingest_frames_ref(s0, 96, 128), ir.ingest_frames_ref(s1, 96, 128)]), c)      # [2, 4, 96, 128, 3]
    trk.open_streams(4)
    slots = [2, 0]
    ref = [trk.track_stream(tensor[:, t0:t0 + 2].contiguous(), slots) for t0 in (0, 2)]
    trk.reset_streams(slots)
    got = [trk.track_stream([d0[t0:t0 + 2], d1[t0:t0 + 2]], slots) for t0 in (0, 2)]
    for call in range(2):
        assert sorted(got[call]) == sorted(ref[call])
        for k in sorted(ref[call]):
            assert torch.equal(got[call][k], ref[call][k]), "call %d: %s differs" % (call, k)
    assert sum(int(r["counts"].sum()) for r in ref) > 0, "vacuous without boxes"
    assert int(ref[1]["nids"].max()) > 0
    with pytest.raises(NativeError):
        trk.track_stream([d0[:2], d1[:1]], slots)          # unequal T
