"""CPU suite: the frame views' definition (include/mi355_dt.h) -- the fit rule and the box-map affine of the library's two
host functions against tests/ingest_view_ref.py and against hand-checked values, the restatement against dt_ingest_frames', and the C and
Python surface as declared."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import ingest_ref as ir
import ingest_view_ref as vr
import mi355_dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(mi355_dt.LIB_PATH), "libmi355_dt.so must be built in-tree (python -m object_tracking_amd.build)"
    L = ctypes.CDLL(mi355_dt.LIB_PATH)
    L.dt_view_fit.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int32)]
    L.dt_view_affine.argtypes = [ctypes.POINTER(mi355_dt.FrameView), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    return L


def c_fit(lib, sw, sh, ow, oh, mode):
    rect = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
    rc = lib.dt_view_fit(sw, sh, ow, oh, mode, rect)
    return rc, tuple(rect)


def c_affine(lib, width, height, crop, dst, out_w, out_h):
    v = mi355_dt.FrameView()
    v.frame.width, v.frame.height = width, height
    v.src_x, v.src_y, v.src_w, v.src_h = crop
    v.dst_x, v.dst_y, v.dst_w, v.dst_h = dst
    a = (ctypes.c_float * 4)()
    assert lib.dt_view_affine(ctypes.byref(v), out_w, out_h, a) == 0
    return np.array(a[:], dtype=np.float32)


# ---- the fit rule ------------------------------------------------------------------------------------------------------------------
BY_HAND = [((1920, 1080, 416, 416), (0, 91, 416, 234)), ((1080, 1920, 416, 416), (91, 0, 234, 416)),
           ((640, 480, 416, 416), (0, 52, 416, 312)), ((1920, 1080, 608, 608), (0, 133, 608, 342))]


def test_fit_values_by_hand(lib):
    for args, want in BY_HAND:
        assert vr.view_fit_ref(*args) == want, args
        assert c_fit(lib, *args, 1) == (0, want), args
        assert mi355_dt.view_fit(*args) == want and mi355_dt.view_fit(*args, mode="letterbox") == want


def test_degenerate_fits_and_stretch(lib):
    # 1 x 5000 into 64 x 64: (1*64 + 2500) / 5000 = 0 -> clamped to 1 pixel, centred with the odd pixel to the right
    assert c_fit(lib, 1, 5000, 64, 64, 1) == (0, (31, 0, 1, 64))
    assert c_fit(lib, 5000, 1, 64, 64, 1) == (0, (0, 31, 64, 1))
    assert c_fit(lib, 1, 1, 1, 1, 1) == (0, (0, 0, 1, 1))
    assert c_fit(lib, 3, 3, 64, 48, 1) == (0, (8, 0, 48, 48))
    assert c_fit(lib, 16384, 16384, 65535, 65535, 1) == (0, (0, 0, 65535, 65535))       # the products need 64 bits
    assert c_fit(lib, 16384, 1, 65535, 65535, 1) == (0, (0, 32765, 65535, 4))           # (65535 + 8192) / 16384 = 4
    for args in ((1920, 1080, 416, 416), (1, 5000, 64, 64), (7, 3, 300, 40)):
        assert c_fit(lib, *args, 0) == (0, (0, 0, args[2], args[3]))
        assert mi355_dt.view_fit(*args, mode="stretch") == (0, 0, args[2], args[3])
    for bad in ((0, 5, 64, 64, 1), (5, 0, 64, 64, 1), (5, 5, 0, 64, 1), (5, 5, 64, 0, 0), (-1, 5, 64, 64, 1), (5, 5, 64, 64, 2), (5, 5, 64, 64, -1)):
        rc, rect = c_fit(lib, *bad)
        assert rc == 1 and rect == (-7, -7, -7, -7), bad            # DT_ERR_ARG, the rectangle untouched
    assert lib.dt_view_fit(5, 5, 64, 64, 1, None) == 1
    with pytest.raises(mi355_dt.NativeError):
        mi355_dt.view_fit(5, 5, 64, 64, mode="pad")
    with pytest.raises(mi355_dt.NativeError):
        mi355_dt.view_fit(0, 5, 64, 64)


def _sweep():
    """a few hundred (width, height, crop, out_w, out_h): round sizes, odd sizes, extreme aspect ratios, random crops"""
    rs = np.random.RandomState(4)
    sizes = [(1920, 1080), (1080, 1920), (1280, 720), (640, 480), (37, 53), (98, 64), (1, 1), (1, 5000), (5000, 1), (16384, 16384), (3, 7), (719, 405)]
    outs = [(416, 416), (608, 608), (64, 64), (300, 40), (96, 128), (1, 1), (13, 999)]
    cases = []
    for W, H in sizes:
        for ow, oh in outs:
            cases.append((W, H, (0, 0, W, H), ow, oh))
            for _ in range(3):
                sw, sh = int(rs.randint(1, W + 1)), int(rs.randint(1, H + 1))
                cases.append((W, H, (int(rs.randint(0, W - sw + 1)), int(rs.randint(0, H - sh + 1)), sw, sh), ow, oh))
    return cases


def test_fit_and_affine_against_the_restatement(lib):
    cases = _sweep()
    assert len(cases) >= 300
    rs = np.random.RandomState(5)
    for W, H, crop, ow, oh in cases:
        for mode in (0, 1):
            want = vr.view_fit_ref(crop[2], crop[3], ow, oh, mode)
            assert c_fit(lib, crop[2], crop[3], ow, oh, mode) == (0, want), (crop, ow, oh, mode)
            x, y, w, h = want
            assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= ow and y + h <= oh
            assert (ow - w) - x in (x, x + 1) and (oh - h) - y in (y, y + 1)          # centred, the odd pixel below / to the right
            if mode == 1:
                assert w == ow or h == oh
            got = c_affine(lib, W, H, crop, want, ow, oh)
            ref = vr.view_affine_ref(W, H, crop, want, ow, oh)
            assert got.tobytes() == ref.tobytes(), (W, H, crop, want, ow, oh, got, ref)
        # an explicit placement somewhere in the output
        dw, dh = int(rs.randint(1, ow + 1)), int(rs.randint(1, oh + 1))
        dst = (int(rs.randint(0, ow - dw + 1)), int(rs.randint(0, oh - dh + 1)), dw, dh)
        assert c_affine(lib, W, H, crop, dst, ow, oh).tobytes() == vr.view_affine_ref(W, H, crop, dst, ow, oh).tobytes()
        v = mi355_dt.FrameView()
        v.frame.width, v.frame.height = W, H
        (v.src_x, v.src_y, v.src_w, v.src_h), (v.dst_x, v.dst_y, v.dst_w, v.dst_h) = crop, dst
        assert mi355_dt.view_affine(v, ow, oh).tobytes() == vr.view_affine_ref(W, H, crop, dst, ow, oh).tobytes()


def test_affine_of_a_stretched_whole_frame_is_exactly_the_identity(lib):
    for W, H, ow, oh in ((1920, 1080, 416, 416), (37, 53, 64, 64), (1, 1, 608, 608), (16384, 16384, 65535, 7), (719, 405, 13, 999)):
        a = c_affine(lib, W, H, (0, 0, W, H), vr.view_fit_ref(W, H, ow, oh, 0), ow, oh)
        assert a.tobytes() == np.array([1, 0, 1, 0], dtype=np.float32).tobytes(), (W, H, ow, oh, a)      # bx, by are +0.0
    v = mi355_dt.FrameView()
    a = (ctypes.c_float * 4)()
    assert lib.dt_view_affine(ctypes.byref(v), 64, 64, a) == 1           # an all-zero view: sizes < 1
    assert lib.dt_view_affine(None, 64, 64, a) == 1


def test_affine_takes_the_destination_corners_to_the_crop_corners(lib):
    """Exact arithmetic: with the exact quotients the corners of the destination rectangle (normalised to the output) land on the
    corners of the crop (normalised to the WHOLE frame).  The definition rounds each of ax, bx once to double (2^-53) and once to float
    (2^-24), relatively: the mapped corner may differ from the crop's by |x * ax| * e + |bx| * e, e = 2^-24 + 2^-52, and by no more."""
    e = Fraction(1, 2 ** 24) + Fraction(1, 2 ** 52)
    checked = 0
    for W, H, crop, ow, oh in _sweep()[::3]:
        dst = vr.view_fit_ref(crop[2], crop[3], ow, oh)
        a = [Fraction(float(v)) for v in c_affine(lib, W, H, crop, dst, ow, oh)]
        exact = [Fraction(n, d) for n, d in vr.affine_ints(W, H, crop, dst, ow, oh)]
        for k in range(4):
            assert abs(a[k] - exact[k]) <= abs(exact[k]) * e
        for axis, (size, out) in enumerate(((W, ow), (H, oh))):
            ax, bx = a[2 * axis], a[2 * axis + 1]
            eax, ebx = exact[2 * axis], exact[2 * axis + 1]
            for corner in (0, 1):
                x = Fraction(dst[axis] + corner * dst[2 + axis], out)
                want = Fraction(crop[axis] + corner * crop[2 + axis], size)
                assert x * eax + ebx == want
                assert abs(x * ax + bx - want) <= (abs(x * eax) + abs(ebx)) * e, (W, H, crop, dst, ow, oh, axis, corner)
                checked += 1
    assert checked >= 400


# ---- the ingest restatement --------------------------------------------------------------------------------------------------------
def test_whole_frame_whole_output_view_is_ingest_frames():
    rs = np.random.RandomState(6)
    items = [rs.randint(0, 256, (37, 53, 3)).astype(np.uint8),
             (rs.randint(0, 256, (36, 52)).astype(np.uint8), rs.randint(0, 256, (18, 26, 2)).astype(np.uint8)),
             rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)]
    views = [vr.View(it, None, (0, 0, 64, 48), (1, 2, 3)) for it in items]
    for swap in (False, True):
        assert np.array_equal(vr.ingest_views_ref(views, 48, 64, swap), ir.ingest_frames_ref(items, 48, 64, swap))


def test_restatement_places_crops_and_fills():
    rs = np.random.RandomState(7)
    rgb = rs.randint(0, 256, (54, 96, 3)).astype(np.uint8)
    out = vr.ingest_views_ref([vr.View(rgb, None, None, (10, 20, 30))], 64, 64, swap_rb=True)[0]
    assert vr.resolve(vr.View(rgb), 64, 64)[1] == (0, 14, 64, 36)
    assert (out[:14] == (10, 20, 30)).all() and (out[50:] == (10, 20, 30)).all()          # the fill is not swapped
    from oracle import oracle as orc
    assert np.array_equal(out[14:50], orc.resize_bilinear_u8(np.ascontiguousarray(rgb[None, :, :, ::-1]), 36, 64)[0])
    # an NV12 crop at an odd origin is the crop of the converted frame: chroma by absolute position
    y, uv = rs.randint(0, 256, (8, 12)).astype(np.uint8), rs.randint(0, 256, (4, 6, 2)).astype(np.uint8)
    got = vr.ingest_views_ref([vr.View((y, uv), (3, 1, 5, 7), (0, 0, 5, 7))], 7, 5)[0]
    assert np.array_equal(got, ir.nv12_to_rgb(y, uv)[1:8, 3:8])


# ---- the box map -------------------------------------------------------------------------------------------------------------------
def test_box_map_inputs_hold_an_element_where_a_fused_multiply_add_differs():
    """x' = x * ax + bx with the product rounded to float32 and then the sum, against ONE rounding of the exact x * ax + bx (what a
    contracted FMA computes): the GPU test's inputs must tell the two apart, or it could not see a contraction."""
    boxes, counts, affine = vr.boxes_map_case()
    ref = vr.boxes_map_ref(boxes, counts, affine)
    differ = 0
    for f in range(boxes.shape[0]):
        for r in range(max(0, min(int(counts[f]), boxes.shape[1]))):
            for k, (a, b) in ((0, (0, 1)), (1, (2, 3))):
                fused = np.float32(float(Fraction(float(boxes[f, r, k])) * Fraction(float(affine[f, a])) + Fraction(float(affine[f, b]))))
                differ += fused.tobytes() != ref[f, r, k].tobytes()
    assert differ >= 1, "no element distinguishes a fused from a separate multiply-add: the GPU test would be vacuous"
    # what the restatement leaves alone, and what -0.0 becomes
    cap = boxes.shape[1]
    for f in range(boxes.shape[0]):
        n = max(0, min(int(counts[f]), cap))
        assert ref[f, n:].tobytes() == boxes[f, n:].tobytes()
        assert ref[f, :, 4:].tobytes() == boxes[f, :, 4:].tobytes()
    assert (counts == 0).any() and (counts > cap).any()
    assert np.signbit(boxes[0, 2, 0]) and not np.signbit(boxes[0, 2, 1])
    assert affine[4].tobytes() == np.array([1, 0, 1, 0], dtype=np.float32).tobytes()
    z = vr.boxes_map_ref(np.full((1, 1, 8), -0.0, dtype=np.float32), [1], affine[4:5])
    assert not np.signbit(z[0, 0, 0]) and np.signbit(z[0, 0, 2]), "-0.0 * 1 + 0 is +0.0: an identity map is not free of effect"


# ---- the C and Python surface ------------------------------------------------------------------------------------------------------
def _decl(hdr, name):
    m = re.search(r"DT_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, "%s is not declared" % name
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    return [re.sub(r"\s*\*\s*", " *", a) for a in args]


def test_header_declares_the_struct_and_the_four_entries():
    hdr = open(os.path.join(ROOT, "include", "mi355_dt.h")).read()
    assert _decl(hdr, "dt_view_fit") == ["int src_w", "int src_h", "int out_w", "int out_h", "int mode", "int32_t rect[4]"]
    assert _decl(hdr, "dt_view_affine") == ["const dt_frame_view *v", "int out_w", "int out_h", "float affine[4]"]
    assert _decl(hdr, "dt_ingest_views") == ["dt_ctx *ctx", "const dt_frame_view *h_views", "int n", "uint8_t *d_dst", "int out_h", "int out_w"]
    assert _decl(hdr, "dt_boxes_map") == ["dt_ctx *ctx", "float *d_boxes", "const int *d_counts", "int n", "int cap", "const float *h_affine"]
    for name, value in (("DT_FIT_STRETCH", 0), ("DT_FIT_LETTERBOX", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
        assert getattr(mi355_dt, name) == value
    m = re.search(r"typedef\s+struct\s+dt_frame_view\s*\{(.*?)\}\s*dt_frame_view\s*;", hdr, re.S)
    assert m, "dt_frame_view is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["dt_frame_desc frame", "int32_t src_x, src_y, src_w, src_h", "int32_t dst_x, dst_y, dst_w, dst_h", "uint8_t fill[3]",
                      "uint8_t reserved0", "int32_t reserved"], fields
    assert re.search(r"1\.08.*?frame-view entries dt_view_fit, dt_view_affine, dt_ingest_views, dt_boxes_map", hdr, re.S)
    for word in ("32 views per launch", "NOT clipped or dropped", "DESIGN.md 4.9c"):
        assert word in hdr, word


def test_binding_lists_the_entries_and_the_struct_is_80_bytes(lib):
    for name in ("dt_view_fit", "dt_view_affine", "dt_ingest_views", "dt_boxes_map"):
        assert name in mi355_dt.SYMBOLS and hasattr(lib, name), name
    V = mi355_dt.FrameView
    assert ctypes.sizeof(V) == 80
    assert [f[0] for f in V._fields_] == ["frame", "src_x", "src_y", "src_w", "src_h", "dst_x", "dst_y", "dst_w", "dst_h", "fill", "reserved0", "reserved"]
    assert (V.src_x.offset, V.dst_x.offset, V.fill.offset, V.reserved0.offset, V.reserved.offset) == (40, 56, 72, 75, 76)
    assert lib.dt_abi_version() == 108
    for name in ("ingest_views", "boxes_map"):
        assert callable(getattr(mi355_dt.Context, name))
    assert callable(mi355_dt.view_fit) and callable(mi355_dt.view_affine)


def test_python_surface_defaults():
    from models_detection.KerasYOLO import KerasYOLO
    from models_tracking.MultiObjDetTracker import MultiObjDetTracker
    from utility import frames
    assert KerasYOLO.INGEST_FIT is None and MultiObjDetTracker.INGEST_FIT is None
    assert callable(frames.ingest_views)
    v = frames.FrameView("frame")
    assert (v.frame, v.crop, v.fit, v.fill, v.dst) == ("frame", None, "letterbox", (128, 128, 128), None)
    v = frames.FrameView("f", crop=(1, 2, 3, 4), fit="stretch", fill=(0, 1, 2), dst=(5, 6, 7, 8))
    assert (v.crop, v.fit, v.fill, v.dst) == ((1, 2, 3, 4), "stretch", (0, 1, 2), (5, 6, 7, 8))
    assert not isinstance(v, (tuple, list))              # a pair is an NV12 item
