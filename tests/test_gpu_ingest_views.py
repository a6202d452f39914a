"""GPU suite (-m gpu): dt_ingest_views and dt_boxes_map -- crops of NV12 / RGB24 frames resized into a rectangle of the network input with a
fill around it, and the decoded boxes taken back to the source frames (include/mi355_dt.h).

Integer arithmetic only in the ingest, one rounded multiply and one rounded add in the box map: bytes are compared exactly and floats as
bits, against dt_ingest_frames where the definition says the two agree and against the plain restatement tests/ingest_view_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

import ingest_ref as ir
import ingest_view_ref as vr
import mi355_dt
from mi355_dt import DT_PIX_NV12, DT_PIX_RGB24, NativeError
from utility import synth
from utility.frames import FrameView, ingest_views

pytestmark = pytest.mark.gpu


def dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def rand_rgb(rs, h, w):
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def rand_nv12(rs, h, w):
    return rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w // 2, 2)).astype(np.uint8)


def to_dev(item, ctx, pitch=None, fill=0xFF):
    """a host item -> the device item; with a pitch the rows lie `pitch` pixels (RGB24) / bytes (NV12) apart in an allocation full of `fill`"""
    if isinstance(item, tuple):
        y, uv = item
        if pitch is None:
            return dev(y, ctx), dev(uv, ctx)
        H, W = y.shape
        ys = np.full((H, pitch), fill, dtype=np.uint8)
        ys[:, :W] = y
        us = np.full((H // 2, pitch), fill, dtype=np.uint8)
        us[:, :W] = uv.reshape(H // 2, W)
        dy, du = dev(ys, ctx), dev(us, ctx)
        return dy[:, :W], du.reshape(-1).as_strided((H // 2, W // 2, 2), (pitch, 2, 1))
    if pitch is None:
        return dev(item, ctx)
    H, W, _ = item.shape
    big = np.full((H, pitch, 3), fill, dtype=np.uint8)
    big[:, :W] = item
    return dev(big, ctx)[:, :W]


def same_bytes(got, ref, what=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = ref.cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.uint8, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError("%s: %d bytes differ, first at %s: got %d, expected %d"
                             % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])]))


def run_views(ctx, views, out_h, out_w, swap_rb=False, pitches=None):
    """views: vr.View on the host -> (device result, device items): every view uploaded (at its pitch) and described with explicit rectangles
    where the host view has them, by the letterbox fit where it has none"""
    d_items = [to_dev(v.item, ctx, pitch=None if pitches is None else pitches[i]) for i, v in enumerate(views)]
    descs = [FrameView(d, crop=v.crop, dst=v.dst, fill=v.fill) for d, v in zip(d_items, views)]
    out, affine = ctx.ingest_views(descs, out_h, out_w, swap_rb=swap_rb)
    assert affine.dtype == np.float32 and affine.tobytes() == vr.views_affine_ref(views, out_h, out_w).tobytes()
    return out, d_items


def check_views(ctx, views, out_h, out_w, swap_rb=False, pitches=None, what=""):
    out, _ = run_views(ctx, views, out_h, out_w, swap_rb, pitches)
    ref = vr.ingest_views_ref(views, out_h, out_w, swap_rb)
    for i in range(len(views)):
        same_bytes(out[i], ref[i], "%s view %d (crop %s, dst %s)" % (what, i, views[i].crop, vr.resolve(views[i], out_h, out_w)[1]))
    return out


# ------------------------------------------------------------------ 1. identity views are dt_ingest_frames
@pytest.mark.parametrize("swap_rb", [False, True], ids=["as_is", "swap_rb"])
def test_identity_views_equal_ingest_frames(ctx, swap_rb):
    rs = np.random.RandomState(1)
    items = [rand_rgb(rs, 37, 53), rand_rgb(rs, 64, 64), rand_rgb(rs, 98, 64), rand_nv12(rs, 64, 64), rand_nv12(rs, 98, 64), rand_rgb(rs, 37, 53)]
    pitches = [None, None, 80, None, 128, 64]
    d_items = [to_dev(a, ctx, pitch=p) for a, p in zip(items, pitches)]
    want = ctx.ingest_frames(d_items, 64, 64, swap_rb=swap_rb)
    got, affine = ctx.ingest_views([FrameView(d, fit="stretch", fill=(9, 8, 7)) for d in d_items], 64, 64, swap_rb=swap_rb)
    same_bytes(got, want, "identity views")
    assert affine.tobytes() == np.tile(np.array([1, 0, 1, 0], dtype=np.float32), (6, 1)).tobytes()
    # plain items with the call's fit, and the module-level helper
    got2, _ = ingest_views(d_items, 64, 64, ctx=ctx, swap_rb=swap_rb, fit="stretch")
    same_bytes(got2, want, "plain items, fit = stretch")
    assert len(np.unique(want.cpu().numpy())) > 100


# ------------------------------------------------------------------ 2. a crop over the whole output is dt_ingest_frames on the offset planes
@pytest.mark.parametrize("swap_rb", [False, True], ids=["as_is", "swap_rb"])
def test_whole_output_crops_equal_ingest_frames_on_offset_planes(ctx, swap_rb):
    rs = np.random.RandomState(2)
    rgb, nv = rand_rgb(rs, 70, 90), rand_nv12(rs, 60, 100)
    d_rgb, (dy, duv) = to_dev(rgb, ctx), to_dev(nv, ctx, pitch=128)
    x, y, w, h = 11, 7, 53, 37                      # RGB24: any origin
    ex, ey, ew, eh = 22, 10, 52, 36                 # NV12 through pointer offsets: an even origin and size
    want = ctx.ingest_frames([d_rgb[y:y + h, x:x + w], (dy[ey:ey + eh, ex:ex + ew], duv[ey // 2:(ey + eh) // 2, ex // 2:(ex + ew) // 2])],
                             64, 48, swap_rb=swap_rb)
    got, affine = ctx.ingest_views([FrameView(d_rgb, crop=(x, y, w, h), fit="stretch"), FrameView((dy, duv), crop=(ex, ey, ew, eh), fit="stretch")],
                                   64, 48, swap_rb=swap_rb)
    same_bytes(got, want, "whole-output crops")
    views = [vr.View(rgb, (x, y, w, h), (0, 0, 48, 64)), vr.View(nv, (ex, ey, ew, eh), (0, 0, 48, 64))]
    same_bytes(got, vr.ingest_views_ref(views, 64, 48, swap_rb), "whole-output crops against the restatement")
    assert affine.tobytes() == vr.views_affine_ref(views, 64, 48).tobytes()


# ------------------------------------------------------------------ 3. letterbox
@pytest.mark.parametrize("swap_rb", [False, True], ids=["as_is", "swap_rb"])
def test_letterbox(ctx, swap_rb):
    rs = np.random.RandomState(3)
    views = [vr.View(rand_rgb(rs, 54, 96), None, None, (10, 130, 250)), vr.View(rand_nv12(rs, 54, 96), None, None, (250, 10, 130)),
             vr.View(rand_rgb(rs, 96, 54), None, None, (130, 250, 10)), vr.View(rand_nv12(rs, 96, 54), None, None, (1, 2, 3))]
    assert [vr.resolve(v, 64, 64)[1] for v in views] == [(0, 14, 64, 36)] * 2 + [(14, 0, 36, 64)] * 2
    out = check_views(ctx, views, 64, 64, swap_rb, pitches=[None, 128, 64, None], what="letterbox").cpu().numpy()
    assert (out[0, :14] == (10, 130, 250)).all() and (out[0, 50:] == (10, 130, 250)).all()      # the fill as it is, swap or not
    assert (out[2, :, :14] == (130, 250, 10)).all() and (out[2, :, 50:] == (130, 250, 10)).all()
    # the same through plain items and the call's fit and fill
    d_items = [to_dev(v.item, ctx) for v in views]
    got, _ = ctx.ingest_views(d_items, 64, 64, swap_rb=swap_rb, fit="letterbox", fill=(4, 5, 6))
    same_bytes(got, vr.ingest_views_ref([v._replace(fill=(4, 5, 6)) for v in views], 64, 64, swap_rb), "plain items, letterbox")


# ------------------------------------------------------------------ 4. odd and tiny crops
def test_odd_and_tiny_crops(ctx):
    rs = np.random.RandomState(4)
    nv, rgb = rand_nv12(rs, 40, 60), rand_rgb(rs, 41, 59)
    guarded = np.full((30, 50, 3), 255, dtype=np.uint8)
    guarded[30 - 9:, 50 - 13:] = 0                                       # the crop is 0, every byte around it (and the pitch padding) 255
    views = [vr.View(nv, (1, 1, 37, 23), None, (1, 2, 3)), vr.View(nv, (21, 3, 5, 35), None, (4, 5, 6)), vr.View(nv, (59, 39, 1, 1), (3, 3, 20, 17)),
             vr.View(rgb, (3, 5, 31, 17), None, (7, 8, 9)), vr.View(rgb, (58, 40, 1, 1), (0, 0, 48, 40)), vr.View(rgb, (0, 0, 1, 1), None),
             vr.View(guarded, (50 - 13, 30 - 9, 13, 9), (2, 2, 40, 30), (77, 77, 77)),
             vr.View(rgb, (20, 20, 5, 5), (1, 0, 47, 40)), vr.View(nv, (7, 9, 5, 5), (0, 0, 48, 40))]
    out = check_views(ctx, views, 40, 48, pitches=[64, None, None, 64, None, None, 64, None, 128], what="odd and tiny").cpu().numpy()
    assert (out[6, 2:32, 2:42] == 0).all(), "a read past the crop pulled a neighbouring 255 in"
    assert (out[2, 3:20, 3:23] == out[2, 3, 3]).all()                    # a 1x1 crop is one colour
    check_views(ctx, views, 40, 48, swap_rb=True, pitches=[64, None, None, 64, None, None, 64, None, 128], what="odd and tiny, swap_rb")


@pytest.mark.parametrize("dst_w", [96, 416, 608])
def test_crop_at_the_widths_where_a_contracted_fma_changes_a_coefficient(ctx, dst_w):
    """a crop of width 32 at src_x = 3 placed at widths 96, 416, 608 ((32, dst_w): tests/test_ingest_frames_cpu.py), as columns and as rows"""
    rs = np.random.RandomState(40 + dst_w)
    ramp = ((np.arange(40)[:, None] * np.array([1, 3, 7])[None, :] + np.array([0, 85, 170])[None, :]) % 256).astype(np.uint8)
    wide = np.ascontiguousarray(np.broadcast_to(ramp[None], (3, 40, 3)))
    views = [vr.View(wide, (3, 1, 32, 2), (5, 1, dst_w, 2), (1, 1, 1)), vr.View(rand_rgb(rs, 3, 40), (3, 0, 32, 3), (0, 0, dst_w, 3)),
             vr.View(rand_nv12(rs, 4, 40), (3, 1, 32, 3), (7, 0, dst_w, 3))]
    check_views(ctx, views, 3, dst_w + 9, what="width 32 -> %d" % dst_w)
    tall = [vr.View(np.ascontiguousarray(v.item.transpose(1, 0, 2)), (v.crop[1], v.crop[0], v.crop[3], v.crop[2]),
                    (v.dst[1], v.dst[0], v.dst[3], v.dst[2]), v.fill) for v in views[:2]]
    check_views(ctx, tall, dst_w + 9, 3, what="height 32 -> %d" % dst_w)


# ------------------------------------------------------------------ 5. placement
def test_placement(ctx):
    rs = np.random.RandomState(5)
    rgb, nv = rand_rgb(rs, 33, 47), rand_nv12(rs, 30, 44)
    views = [vr.View(rgb, None, (137, 0, 1, 40), (1, 2, 3)),              # one pixel wide
             vr.View(nv, (1, 1, 41, 27), (299, 39, 1, 1), (4, 5, 6)),     # one pixel, the last of the output
             vr.View(rgb, (2, 3, 40, 20), (0, 0, 30, 12), (7, 8, 9)),     # the top left corner
             vr.View(nv, None, (270, 22, 30, 18), (10, 11, 12)),          # the bottom right corner
             vr.View(rgb, None, (200, 5, 90, 30), (13, 14, 15)),          # straddling column 256: two column blocks
             vr.View(nv, (3, 1, 39, 29), (255, 0, 2, 40), (16, 17, 18)),  # columns 255 and 256
             vr.View(rgb, None, (0, 0, 300, 40), (19, 20, 21))]           # no fill at all
    for swap in (False, True):
        check_views(ctx, views, 40, 300, swap, what="placement")


# ------------------------------------------------------------------ 6. more views than one launch carries
def many_views(n, seed, out_h, out_w):
    rs = np.random.RandomState(seed)
    views = []
    for i in range(n):
        h, w = 8 + 2 * (i % 4), 10 + 2 * (i % 3)
        item = rand_nv12(rs, h, w) if i % 2 else rand_rgb(rs, h + 1, w - 1)
        W, H = vr.item_size(item)
        sw, sh = 1 + i % W, 1 + (3 * i) % H
        dw, dh = 1 + (5 * i) % out_w, 1 + (7 * i) % out_h
        views.append(vr.View(item, ((i * 3) % (W - sw + 1), (i * 5) % (H - sh + 1), sw, sh),
                             ((i * 7) % (out_w - dw + 1), (i * 11) % (out_h - dh + 1), dw, dh), (i, 255 - i, (37 * i) % 256)))
    return views


def test_more_views_than_one_launch():
    """35 views at 32 per launch, each with its own crop, placement and fill: two launches under the "ingest" name, with the algorithmic
    bytes of the SOURCE RECTANGLES (1.5 per NV12 pixel, 3 per RGB24 pixel) and the 3 * out_h * out_w written per frame"""
    c = mi355_dt.Context()
    try:
        views = many_views(35, 6, 24, 40)
        assert len({(v.crop, v.dst, v.fill) for v in views}) == 35
        d_items = [to_dev(v.item, c) for v in views]
        descs = [FrameView(d, crop=v.crop, dst=v.dst, fill=v.fill) for d, v in zip(d_items, views)]
        c.profile_reset(); c.profile_enable(True)
        out, _ = c.ingest_views(descs, 24, 40)
        c.profile_enable(False)
        p = c.profile_read("ingest")
        ref = vr.ingest_views_ref(views, 24, 40)
        for i in range(35):
            same_bytes(out[i], ref[i], "view %d of 35" % i)
        want = sum((1.5 if isinstance(v.item, tuple) else 3.0) * v.crop[2] * v.crop[3] for v in views) + 35 * 3.0 * 24 * 40
        assert p["launches"] == 2, p
        assert p["bytes"] == want, (p, want)
        c.profile_reset(); c.profile_enable(True)
        c.ingest_views(descs[:32], 24, 40)
        c.profile_enable(False)
        assert c.profile_read("ingest")["launches"] == 1
    finally:
        c.close()


# ------------------------------------------------------------------ 7. errors
def _view(p0, p1, h, w, pitch0, pitch1, fmt, src, dst, fill=(1, 2, 3), reserved0=0, reserved=0, desc_reserved=0):
    return mi355_dt.FrameView(mi355_dt.FrameDesc(p0, p1, h, w, pitch0, pitch1, fmt, desc_reserved), src[0], src[1], src[2], src[3],
                              dst[0], dst[1], dst[2], dst[3], (ctypes.c_uint8 * 3)(*fill), reserved0, reserved)


def test_errors_leave_the_destination_untouched(ctx):
    t = torch
    buf = t.zeros(1 << 14, dtype=t.uint8, device=ctx.device)
    P = buf.data_ptr()
    dst = t.full((33, 16, 20, 3), 0xA5, dtype=t.uint8, device=ctx.device)
    D = ctypes.c_void_p(dst.data_ptr())
    rgb = lambda src=(0, 0, 8, 8), d=(0, 0, 20, 16), **kw: _view(P, None, 8, 8, 24, 0, DT_PIX_RGB24, src, d, **kw)
    nv = lambda src=(0, 0, 8, 8), d=(0, 0, 20, 16), **kw: _view(P, P + 4096, 8, 8, 8, 8, DT_PIX_NV12, src, d, **kw)
    lib, h = ctx.lib, ctx.h
    ctx._sync_stream()

    def call(views, n=None, d=D, oh=16, ow=20, handle=h, null_views=False):
        arr = (mi355_dt.FrameView * max(1, len(views)))(*views)
        rc = lib.dt_ingest_views(handle, None if null_views else arr, len(views) if n is None else n, d, oh, ow)
        return rc, lib.dt_last_error(handle).decode()

    assert call([rgb(), nv(), rgb((7, 7, 1, 1), (19, 15, 1, 1)), nv((1, 1, 7, 7), (0, 0, 1, 16))])[0] == 0      # the templates, and rectangles that just fit
    t.cuda.synchronize()
    dst.fill_(0xA5)
    for kw in (dict(handle=None), dict(null_views=True), dict(d=None), dict(n=0), dict(n=-1), dict(oh=0), dict(ow=0), dict(oh=65536)):
        assert call([rgb()], **kw)[0] == 1, kw
    bad = {
        "source one pixel beyond the width": rgb((1, 0, 8, 8)),
        "source one pixel beyond the height": nv((0, 1, 8, 8)),
        "source x -1": rgb((-1, 0, 8, 8)),
        "source y -1": rgb((0, -1, 4, 4)),
        "source width 0": rgb((0, 0, 0, 8)),
        "source height 0": nv((0, 0, 8, 0)),
        "source width -1": rgb((4, 0, -1, 8)),
        "source width wraps": rgb((2, 0, 2 ** 31 - 1, 8)),
        "destination one pixel beyond the width": rgb(d=(1, 0, 20, 16)),
        "destination one pixel beyond the height": nv(d=(0, 1, 20, 16)),
        "destination x -1": rgb(d=(-1, 0, 4, 4)),
        "destination width 0": rgb(d=(0, 0, 0, 16)),
        "destination height 0": nv(d=(0, 0, 20, 0)),
        "destination width wraps": rgb(d=(2, 0, 2 ** 31 - 1, 16)),
        "reserved 1": rgb(reserved=1),
        "reserved0 1": nv(reserved0=1),
        "descriptor reserved 1": rgb(desc_reserved=1),
        "null plane0": _view(None, None, 8, 8, 24, 0, DT_PIX_RGB24, (0, 0, 8, 8), (0, 0, 20, 16)),
        "NV12 odd width": _view(P, P + 4096, 8, 7, 8, 8, DT_PIX_NV12, (0, 0, 7, 8), (0, 0, 20, 16)),
        "pitch0 below a row": _view(P, None, 8, 8, 23, 0, DT_PIX_RGB24, (0, 0, 8, 8), (0, 0, 20, 16)),
        "unknown format": _view(P, None, 8, 8, 24, 0, 2, (0, 0, 8, 8), (0, 0, 20, 16)),
    }
    for name, v in sorted(bad.items()):
        rc, msg = call([rgb(), nv(), v, rgb()])
        assert rc == 1, name
        assert "frame 2" in msg, (name, msg)
    # only the LAST view of a 33-view call is bad: nothing of the first launch's 32 views is written either
    rc, msg = call([rgb(), nv()] * 16 + [bad["destination height 0"]])
    assert rc == 1 and "frame 32" in msg, msg
    t.cuda.synchronize()
    assert bool((dst == 0xA5).all()), "an error wrote to the destination"
    # dt_boxes_map's own
    boxes = t.zeros((2, 4, 8), dtype=t.float32, device=ctx.device)
    counts = t.ones((2,), dtype=t.int32, device=ctx.device)
    ok = np.array([[1, 0, 1, 0], [2, 1, 2, 1]], dtype=np.float32)
    B, C, A = ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(counts.data_ptr()), ok.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, B, C, 2, 4, A), (h, None, C, 2, 4, A), (h, B, None, 2, 4, A), (h, B, C, 2, 4, None), (h, B, C, 0, 4, A), (h, B, C, -1, 4, A), (h, B, C, 2, 0, A)):
        assert lib.dt_boxes_map(*args) == 1, args
    for k, v in ((1, np.nan), (4, np.inf), (7, -np.inf)):
        a = ok.copy()
        a.reshape(-1)[k] = v
        assert lib.dt_boxes_map(h, B, C, 2, 4, a.ctypes.data_as(ctypes.c_void_p)) == 1
        assert "frame %d" % (k // 4) in lib.dt_last_error(h).decode()
    t.cuda.synchronize()
    assert bool((boxes == 0).all())


def test_python_items_are_checked(ctx):
    t = torch
    ok = t.zeros((8, 8, 3), dtype=t.uint8, device=ctx.device)
    y, uv = t.zeros((8, 8), dtype=t.uint8, device=ctx.device), t.zeros((4, 4, 2), dtype=t.uint8, device=ctx.device)
    bad = {
        "host frame": FrameView(ok.cpu()),
        "numpy frame": np.zeros((8, 8, 3), dtype=np.uint8),
        "float frame": FrameView(ok.float()),
        "pair of three": FrameView((y, uv, uv)),
        "crop of three": FrameView(ok, crop=(0, 0, 8)),
        "crop of floats": FrameView(ok, crop=(0, 0, 7.5, 8)),
        "crop not a sequence": FrameView(ok, crop=5),
        "empty crop": FrameView(ok, crop=(0, 0, 0, 8)),
        "crop outside": FrameView((y, uv), crop=(1, 0, 8, 8)),
        "dst outside": FrameView(ok, dst=(0, 1, 16, 16)),
        "dst of five": FrameView(ok, dst=(0, 0, 1, 1, 1)),
        "unknown fit": FrameView(ok, fit="pad"),
        "fill of two": FrameView(ok, fill=(1, 2)),
        "fill 256": FrameView((y, uv), fill=(0, 0, 256)),
        "fill -1": FrameView(ok, fill=(0, -1, 0)),
    }
    for name, item in sorted(bad.items()):
        with pytest.raises(NativeError) as e:
            ctx.ingest_views([ok, FrameView((y, uv)), item], 16, 16)
        assert "frame 2" in str(e.value) and "dt_ingest_views" in str(e.value), (name, str(e.value))
    with pytest.raises(NativeError):
        ctx.ingest_views(ok[None], 16, 16)                  # a tensor is not a list of views
    with pytest.raises(NativeError):
        ctx.ingest_views([ok], 16, 16, fit="pad")
    with pytest.raises(NativeError):
        ctx.ingest_views([ok], 16, 16, out=t.empty((1, 16, 16, 3), dtype=t.uint8, device=ctx.device)[:, :, ::2])
    boxes, counts = t.zeros((2, 3, 4, 8), dtype=t.float32, device=ctx.device), t.zeros((2, 3), dtype=t.int32, device=ctx.device)
    with pytest.raises(NativeError):
        ctx.boxes_map(boxes, counts, np.zeros((5, 4), dtype=np.float32))        # 6 frames, 5 affines
    with pytest.raises(NativeError):
        ctx.boxes_map(boxes, counts[:1], np.zeros((6, 4), dtype=np.float32))
    # out: a slice of a batch is filled in place
    batch = t.full((2, 2, 16, 16, 3), 0xA5, dtype=t.uint8, device=ctx.device)
    rs = np.random.RandomState(9)
    views = [vr.View(rand_rgb(rs, 5, 9)), vr.View(rand_nv12(rs, 6, 4), (1, 1, 3, 4))]
    ret, _ = ctx.ingest_views([FrameView(to_dev(v.item, ctx), crop=v.crop) for v in views], 16, 16, out=batch[1])
    assert ret.data_ptr() == batch[1].data_ptr()
    same_bytes(batch[1], vr.ingest_views_ref(views, 16, 16), "out=")
    assert bool((batch[0] == 0xA5).all())


# ------------------------------------------------------------------ 8. the box map
def test_boxes_map(ctx):
    boxes, counts, affine = vr.boxes_map_case()
    ref = vr.boxes_map_ref(boxes, counts, affine)
    d_boxes, d_counts = dev(boxes, ctx), dev(counts, ctx)
    ret = ctx.boxes_map(d_boxes, d_counts, affine)
    assert ret.data_ptr() == d_boxes.data_ptr()                         # in place
    got = d_boxes.cpu().numpy()
    gb, rb = got.view(np.uint32), ref.view(np.uint32)
    assert np.array_equal(gb, rb), "first differing (frame, row, float): %s" % np.argwhere(gb != rb)[:4].tolist()
    cap = boxes.shape[1]
    src = boxes.view(np.uint32)
    for f in range(len(counts)):
        n = max(0, min(int(counts[f]), cap))
        assert np.array_equal(gb[f, n:], src[f, n:]), "frame %d: a row beyond the count changed" % f
        assert np.array_equal(gb[f, :, 4:], src[f, :, 4:]), "frame %d: floats 4..7 changed" % f
    assert (gb[:, :, :4] != src[:, :, :4]).any()
    # [R, T, cap, 8] counts as R * T frames; more frames than one launch's arguments hold (128)
    rs = np.random.RandomState(82)
    big = rs.uniform(-0.25, 1.25, (65, 2, 3, 8)).astype(np.float32)
    bc = rs.randint(0, 5, (65, 2)).astype(np.int32)
    ba = np.stack([affine[i % len(affine)] * np.float32(1 + i % 3) for i in range(130)])
    want = vr.boxes_map_ref(big, bc, ba)
    got = ctx.boxes_map(dev(big, ctx), dev(bc, ctx), ba).cpu().numpy()
    assert got.shape == big.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------ 9. fresh versus used context
def test_fresh_and_used_context_agree():
    from oracle import oracle as orc
    rs = np.random.RandomState(10)
    views = [vr.View(rand_nv12(rs, 36, 52), (5, 3, 41, 29), None, (1, 2, 3)), vr.View(rand_rgb(rs, 21, 17), None, (3, 4, 30, 40)),
             vr.View(rand_nv12(rs, 2, 2))]

    def target(c):
        return run_views(c, views, 48, 40, pitches=[64, 64, None])[0].cpu().numpy()

    fresh = mi355_dt.Context()
    try:
        want = target(fresh)
    finally:
        fresh.close()
    used = mi355_dt.Context()
    try:
        src = rs.randint(0, 256, (2, 37, 53, 3)).astype(np.uint8)
        d_src = dev(src, used)
        first = used.ingest_resize(d_src, 48, 40).cpu().numpy()
        run_views(used, many_views(40, 11, 96, 128), 96, 128)
        used.ingest_frames([to_dev(rand_rgb(rs, 50, 60), used)], 30, 30)
        got = target(used)
        third = used.ingest_resize(d_src, 48, 40).cpu().numpy()          # dt_ingest_resize's cached table was left alone
    finally:
        used.close()
    assert np.array_equal(got, want)
    same_bytes(want, vr.ingest_views_ref(views, 48, 40), "fresh context")
    assert np.array_equal(first, third) and np.array_equal(first, orc.resize_bilinear_u8(src, 48, 40))


# ------------------------------------------------------------------ 10. / 11. plumbing
@pytest.fixture(scope="module")
def small_tracker():
    """96x128 (3x4 grid), C = 12, head scaled so that frames carry boxes (as tests/test_gpu_ingest_frames.py builds it)"""
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


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def test_detect_on_letterboxed_lists(monkeypatch, small_tracker):
    det = small_tracker.detector
    monkeypatch.setattr(det, "OBJ_THRESHOLD", 0.02, raising=False)
    c = det.model.ctx
    rs = np.random.RandomState(12)
    items = [rand_nv12(rs, 120, 160), rand_rgb(rs, 200, 90), rand_nv12(rs, 54, 250), rand_rgb(rs, 96, 128)]
    d_items = [to_dev(items[0], c, pitch=192), to_dev(items[1], c, pitch=96), to_dev(items[2], c), to_dev(items[3], c)]
    # today's path, key for key
    assert det.INGEST_FIT is None
    plain = det.detect(d_items)
    ref_plain = det.detect(dev(ir.ingest_frames_ref(items, 96, 128), c))
    assert sorted(plain) == sorted(ref_plain) == ["boxes", "classes", "counts", "post"]
    assert np.array_equal(bits(plain["boxes"]), bits(ref_plain["boxes"])) and torch.equal(plain["counts"], ref_plain["counts"])
    # letterboxed: plain items by the class's rule, and one explicit view with a crop
    monkeypatch.setattr(det, "INGEST_FIT", "letterbox", raising=False)
    given = d_items[:3] + [FrameView(d_items[3], crop=(11, 5, 90, 40), fill=(0, 0, 0))]
    views = [vr.View(it) for it in items[:3]] + [vr.View(items[3], (11, 5, 90, 40), None, (0, 0, 0))]
    got = det.detect(given)
    ref = det.detect(dev(vr.ingest_views_ref(views, 96, 128), c))
    affine = vr.views_affine_ref(views, 96, 128)
    assert sorted(got) == ["affine", "boxes", "classes", "counts", "post"] and "affine" not in ref
    assert got["affine"].tobytes() == affine.tobytes()
    assert torch.equal(got["counts"], ref["counts"])
    want = vr.boxes_map_ref(ref["boxes"].cpu().numpy(), ref["counts"].cpu().numpy(), affine)
    assert np.array_equal(bits(got["boxes"]), bits(want))
    n = int(ref["counts"].sum())
    print("detect, letterboxed: %d boxes" % n)
    assert n > 0, "vacuous without boxes"
    assert not np.array_equal(bits(got["boxes"]), bits(ref["boxes"]))


@pytest.mark.parametrize("min_hits", [None, 1], ids=["ids", "readout"])
def test_track_stream_on_letterboxed_lists(monkeypatch, small_tracker, min_hits):
    """two streams x 3 frames of different source sizes: the result equals that of the pre-ingested tensor with the boxes mapped to
    source coordinates BEFORE the association -- ids and, with MIN_HITS, the read-out rows, which then live in source space"""
    trk = small_tracker
    c = trk.model.ctx
    monkeypatch.setattr(trk, "INGEST_FIT", "letterbox", raising=False)
    if min_hits is not None:
        monkeypatch.setattr(trk, "MIN_HITS", min_hits, raising=False)
        monkeypatch.setattr(trk, "MAX_AGE", 2, raising=False)
        monkeypatch.setattr(trk, "MOTION_GAIN", 0.5, raising=False)
    rs = np.random.RandomState(13)
    s0 = [rand_nv12(rs, 120, 160), rand_nv12(rs, 90, 200), rand_nv12(rs, 120, 160)]
    s1 = [np.ascontiguousarray(f) for f in synth.synth_clip(3, 140, 100, 2, seed=14)]
    d0 = [to_dev(a, c, pitch=256) for a in s0]
    d1 = [to_dev(a, c, pitch=128) for a in s1]
    views = [vr.View(a) for a in s0 + s1]
    tensor = dev(vr.ingest_views_ref(views, 96, 128).reshape(2, 3, 96, 128, 3), c)
    affine = vr.views_affine_ref(views, 96, 128)
    slots = [1, 3]
    trk.open_streams(4)
    got = trk.track_stream([d0, d1], slots)
    # the same by hand from fresh slots: forward, decode, the restatement's box map on the host, then the class's association
    trk.reset_streams(slots)
    cap = got["boxes"].shape[2]
    net = trk.model.forward_stream(tensor, slots, want_det=False)
    r = c.decode(net.reshape((6,) + tuple(net.shape[2:])), trk.OBJ_THRESHOLD, trk.NMS_THRESHOLD, trk.ANCHORS, len(trk.LABELS), cap=cap)
    counts = r["counts"].reshape(2, 3)
    mapped = dev(vr.boxes_map_ref(r["boxes"].cpu().numpy(), r["counts"].cpu().numpy(), affine).reshape(2, 3, cap, 8), c)
    ref = trk._associate_stream(mapped, counts, slots)
    assert sorted(got) == sorted(list(ref) + ["netout", "affine"])
    assert got["affine"].shape == (2, 3, 4) and got["affine"].tobytes() == affine.tobytes()
    assert torch.equal(got["netout"], net)
    for k in sorted(ref):
        assert np.array_equal(bits(got[k]), bits(ref[k])), "%s differs" % k
    assert int(counts.sum()) > 0 and int(ref["nids"].max()) > 0, "vacuous without boxes"
    assert not np.array_equal(bits(got["boxes"]), bits(r["boxes"].reshape(2, 3, cap, 8)))
    if min_hits is not None:
        assert "tracks" in ref and int(ref["track_counts"].sum()) > 0
    trk.reset_streams(slots)
