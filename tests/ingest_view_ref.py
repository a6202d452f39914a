"""Plain restatement of the frame views (include/mi355_dt.h) in Python / numpy: test infrastructure only.

The fit rule and the affine in Python integers, the box map in numpy float32 (every multiply and every add rounded on its own), and the
view ingest as  crop(ingest_ref.convert(item))  ->  the ORACLE's resize to the destination rectangle  ->  pasted onto a canvas of the fill.
"""
import collections

import numpy as np

import ingest_ref as ir

STRETCH, LETTERBOX = 0, 1

# one view on the host: item as ingest_ref takes it, crop / dst = (x, y, w, h) or None (the whole frame / the letterbox fit), fill = 3 bytes
View = collections.namedtuple("View", "item crop dst fill")
View.__new__.__defaults__ = (None, None, (128, 128, 128))


def item_size(item):
    """(width, height) of a host item"""
    a = item[0] if isinstance(item, (tuple, list)) else item
    return int(a.shape[1]), int(a.shape[0])


def view_fit_ref(src_w, src_h, out_w, out_h, mode=LETTERBOX):
    """(x, y, w, h): Python integers, // on non-negative values is the truncating division of the definition"""
    assert min(src_w, src_h, out_w, out_h) >= 1 and mode in (STRETCH, LETTERBOX)
    if mode == STRETCH:
        return (0, 0, out_w, out_h)
    if src_w * out_h >= src_h * out_w:
        w, h = out_w, max(1, (src_h * out_w + src_w // 2) // src_w)
    else:
        w, h = max(1, (src_w * out_h + src_h // 2) // src_h), out_h
    return ((out_w - w) // 2, (out_h - h) // 2, w, h)


def resolve(view, out_h, out_w):
    """-> (crop, dst) with the defaults filled in"""
    W, H = item_size(view.item)
    crop = (0, 0, W, H) if view.crop is None else tuple(int(v) for v in view.crop)
    dst = view_fit_ref(crop[2], crop[3], out_w, out_h) if view.dst is None else tuple(int(v) for v in view.dst)
    return crop, dst


def affine_ints(width, height, crop, dst, out_w, out_h):
    """the four exact quotients (numerator, denominator) of (ax, bx, ay, by)"""
    sx, sy, sw, sh = crop
    dx, dy, dw, dh = dst
    return [(out_w * sw, dw * width), (sx * dw - dx * sw, dw * width), (out_h * sh, dh * height), (sy * dh - dy * sh, dh * height)]


def view_affine_ref(width, height, crop, dst, out_w, out_h):
    """float32 [4]: integer products, ONE double division (Python's float / float on exactly converted integers), ONE rounding to float"""
    out = np.empty(4, dtype=np.float32)
    for k, (num, den) in enumerate(affine_ints(width, height, crop, dst, out_w, out_h)):
        assert abs(num) < 2 ** 53 and 0 < den < 2 ** 53
        out[k] = np.float32(float(num) / float(den))
    return out


def views_affine_ref(views, out_h, out_w):
    out = np.empty((len(views), 4), dtype=np.float32)
    for i, v in enumerate(views):
        W, H = item_size(v.item)
        crop, dst = resolve(v, out_h, out_w)
        out[i] = view_affine_ref(W, H, crop, dst, out_w, out_h)
    return out


def boxes_map_ref(boxes, counts, affine):
    """boxes float32 [..., cap, 8], counts int [...], affine float32 [frames, 4] -> a mapped copy.  numpy float32 arithmetic rounds after
    every operation: the product first, then the sum.  Rows from min(count, cap) on and floats 4..7 are copied bit for bit."""
    boxes = np.asarray(boxes)
    assert boxes.dtype == np.float32 and boxes.shape[-1] == 8
    cap = boxes.shape[-2]
    out = boxes.copy().reshape(-1, cap, 8)
    src = boxes.reshape(-1, cap, 8)
    cnt = np.asarray(counts).reshape(-1)
    aff = np.asarray(affine, dtype=np.float32).reshape(-1, 4)
    assert len(cnt) == len(aff) == out.shape[0]
    for f in range(out.shape[0]):
        n = max(0, min(int(cnt[f]), cap))
        ax, bx, ay, by = (np.float32(v) for v in aff[f])
        r = src[f, :n]
        out[f, :n, 0] = (r[:, 0] * ax).astype(np.float32) + bx
        out[f, :n, 1] = (r[:, 1] * ay).astype(np.float32) + by
        out[f, :n, 2] = r[:, 2] * ax
        out[f, :n, 3] = r[:, 3] * ay
    assert out.dtype == np.float32
    return out.reshape(boxes.shape)


def ingest_views_ref(views, out_h, out_w, swap_rb=False):
    """views -> uint8 [n, out_h, out_w, 3]"""
    from oracle import oracle as orc
    out = np.empty((len(views), out_h, out_w, 3), dtype=np.uint8)
    for i, v in enumerate(views):
        (sx, sy, sw, sh), (dx, dy, dw, dh) = resolve(v, out_h, out_w)
        conv = ir.convert(v.item, swap_rb)
        assert 0 <= sx and 0 <= sy and sw >= 1 and sh >= 1 and sx + sw <= conv.shape[1] and sy + sh <= conv.shape[0], (v.crop, conv.shape)
        assert 0 <= dx and 0 <= dy and dw >= 1 and dh >= 1 and dx + dw <= out_w and dy + dh <= out_h, (v.dst, out_h, out_w)
        crop = np.ascontiguousarray(conv[sy:sy + sh, sx:sx + sw])
        out[i] = np.asarray(v.fill, dtype=np.uint8)[None, None, :]           # the fill as it is: the swap is the frame's
        out[i, dy:dy + dh, dx:dx + dw] = orc.resize_bilinear_u8(crop[None], dh, dw)[0]
    return out


def boxes_map_case():
    """The inputs of the GPU test of dt_boxes_map, seeded: boxes [7, 12, 8] with -0.0, NaN patterns beyond the counts, counts with 0 and
    one above the capacity, and the affines of letterboxed and cropped views (tests/test_ingest_views_cpu.py holds them to contain an
    element where a fused multiply-add would give other bits)."""
    rs = np.random.RandomState(81)
    n, cap = 7, 12
    boxes = rs.uniform(-0.25, 1.25, (n, cap, 8)).astype(np.float32)
    counts = np.array([5, 0, 12, 15, 1, 7, 3], dtype=np.int32)
    boxes[0, 1, 0] = -0.0
    boxes[0, 2, :4] = (-0.0, 0.0, -0.0, 0.0)
    boxes[2, 3, 1] = -0.0
    bits = boxes.view(np.uint32)
    for f in range(n):
        for r in range(max(0, min(int(counts[f]), cap)), cap):
            bits[f, r] = 0x7FC00000 + 0x101 * (f * cap + r) + np.arange(8)      # quiet NaNs with distinct payloads
    affine = np.stack([
        view_affine_ref(1920, 1080, (0, 0, 1920, 1080), view_fit_ref(1920, 1080, 416, 416), 416, 416),
        view_affine_ref(1080, 1920, (0, 0, 1080, 1920), view_fit_ref(1080, 1920, 416, 416), 416, 416),
        view_affine_ref(1920, 1080, (481, 271, 959, 539), view_fit_ref(959, 539, 416, 416), 416, 416),
        view_affine_ref(640, 480, (3, 5, 33, 77), (17, 9, 100, 50), 608, 608),
        view_affine_ref(64, 64, (0, 0, 64, 64), (0, 0, 64, 64), 64, 64),               # the identity: (1, 0, 1, 0)
        view_affine_ref(98, 64, (1, 1, 97, 63), view_fit_ref(97, 63, 64, 64), 64, 64),
        view_affine_ref(1280, 720, (0, 0, 1280, 720), view_fit_ref(1280, 720, 608, 608), 608, 608),
    ])
    return boxes, counts, affine
