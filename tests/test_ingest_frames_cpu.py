"""CPU suite: dt_ingest_frames' definition as tests/ingest_ref.py restates it (the NV12 -> RGB conversion), the decoder-surface views of
utility/frames.py, and the C surface as the header declares it."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import torch

import ingest_ref as ir
import mi355_dt
from utility.frames import nv12_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Y, U, V) -> (R, G, B), checked by hand from the formula in include/mi355_dt.h
VALUES = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((126, 128, 128), (128, 128, 128)),
          ((81, 90, 240), (254, 0, 0)), ((145, 54, 34), (0, 255, 1)), ((41, 240, 110), (0, 0, 255)),
          ((0, 0, 0), (0, 154, 0)), ((255, 255, 255), (255, 125, 255)), ((255, 0, 0), (74, 255, 20))]


def _one(Y, U, V):
    y = np.full((2, 2), Y, dtype=np.uint8)
    uv = np.array([[[U, V]]], dtype=np.uint8)
    return y, uv


def test_value_table():
    for (Y, U, V), rgb in VALUES:
        got = ir.nv12_to_rgb(*_one(Y, U, V))
        assert got.shape == (2, 2, 3) and got.dtype == np.uint8
        assert (got == np.array(rgb, dtype=np.uint8)).all(), ((Y, U, V), got[0, 0].tolist(), rgb)


def test_both_clamps_are_reached_and_int32_holds_the_sums():
    rs = np.random.RandomState(5)
    y = rs.randint(0, 256, (64, 96)).astype(np.uint8)
    uv = rs.randint(0, 256, (32, 48, 2)).astype(np.uint8)
    raw = ir.nv12_to_rgb_unclamped(y, uv)
    for ch in range(3):
        assert raw[..., ch].min() < 0 and raw[..., ch].max() > 255, "channel %d never leaves [0, 255] before the clamp" % ch
    got = ir.nv12_to_rgb(y, uv)
    assert got.min() == 0 and got.max() == 255
    assert np.array_equal(got, np.clip(raw, 0, 255).astype(np.uint8))
    # the extreme intermediate sums the header's formula can reach, in Python integers
    hi = max(239 * 1220542 + 2116026 * 127 + 524288, 239 * 1220542 + 1673527 * 127 + 524288)
    lo = min(-1673527 * 128 + 524288, -2116026 * 128 + 524288, -852492 * 127 - 409993 * 127 + 524288)
    assert (hi, lo) == (560969128, -270327040)
    assert hi < 2 ** 31 and lo > -2 ** 31
    assert int(raw.max()) <= hi >> 20 and int(raw.min()) >= lo >> 20


def test_a_2x2_block_shares_its_chroma():
    rs = np.random.RandomState(6)
    y = np.full((4, 6), 120, dtype=np.uint8)              # one luma everywhere: what differs between pixels is the chroma alone
    uv = rs.randint(0, 256, (2, 3, 2)).astype(np.uint8)
    got = ir.nv12_to_rgb(y, uv)
    for r in range(2):
        for c in range(3):
            blk = got[2 * r:2 * r + 2, 2 * c:2 * c + 2].reshape(4, 3)
            assert (blk == blk[0]).all(), (r, c)
            assert (blk[0] == ir.nv12_to_rgb(*_one(120, uv[r, c, 0], uv[r, c, 1]))[0, 0]).all()
    assert len({tuple(got[2 * r, 2 * c]) for r in range(2) for c in range(3)}) > 1, "every block got the same colour: vacuous"


def test_swap_and_resize_of_the_restatement():
    from oracle import oracle as orc
    rs = np.random.RandomState(7)
    rgb = rs.randint(0, 256, (10, 14, 3)).astype(np.uint8)
    y = rs.randint(0, 256, (8, 12)).astype(np.uint8)
    uv = rs.randint(0, 256, (4, 6, 2)).astype(np.uint8)
    out = ir.ingest_frames_ref([rgb, (y, uv)], 16, 16)
    assert np.array_equal(out[0], orc.resize_bilinear_u8(rgb[None], 16, 16)[0])
    assert np.array_equal(out[1], orc.resize_bilinear_u8(ir.nv12_to_rgb(y, uv)[None], 16, 16)[0])
    assert np.array_equal(ir.ingest_frames_ref([rgb, (y, uv)], 16, 16, swap_rb=True), out[..., ::-1])


def test_nv12_planes_are_views_of_the_surface():
    H, W, P = 6, 8, 16
    surface = torch.arange((H + H // 2) * P, dtype=torch.int32).to(torch.uint8)
    y, uv = nv12_planes(surface, H, W, pitch=P)
    assert tuple(y.shape) == (H, W) and tuple(y.stride()) == (P, 1)
    assert tuple(uv.shape) == (H // 2, W // 2, 2) and tuple(uv.stride()) == (P, 2, 1)
    assert y.data_ptr() == surface.data_ptr() and uv.data_ptr() == surface.data_ptr() + H * P      # no copy
    s = surface.numpy().reshape(H + H // 2, P)
    assert np.array_equal(y.numpy(), s[:H, :W])
    assert np.array_equal(uv.numpy(), s[H:, :W].reshape(H // 2, W // 2, 2))
    surface[2 * P + 3] = 201                 # a write to the surface shows in the views
    surface[(H + 1) * P + 5] = 202
    assert int(y[2, 3]) == 201 and int(uv[1, 2, 1]) == 202
    y2, uv2 = nv12_planes(surface[:(H + H // 2) * W], H, W)      # default pitch: the width
    assert tuple(y2.stride()) == (W, 1) and tuple(uv2.stride()) == (W, 2, 1)
    for bad in (dict(height=5, width=8), dict(height=6, width=7), dict(height=6, width=8, pitch=7), dict(height=8, width=8, pitch=16)):
        try:
            nv12_planes(surface, **bad)
        except ValueError:
            continue
        raise AssertionError("nv12_planes accepted %r" % bad)


# ---- the coefficient formula: where a fused multiply-subtract would differ --------------------------------------------------------
COEF_PAIRS = [(1080, 416), (1920, 416), (37, 64), (53, 64), (98, 64), (719, 608), (64, 64), (1, 5), (7, 3)]
FMA_PAIRS = [(32, 96), (32, 416), (32, 608)]


def _f_separate_and_fused(src, dst):
    """f = (float)((d + 0.5) * scale - 0.5) for every d: product and subtraction rounded one by one (ingest_tables), and as ONE rounded
    operation (what a contracted FMA computes; exact rational arithmetic, then one rounding to double)"""
    scale = src / dst
    sep = np.array([np.float32((d + 0.5) * scale - 0.5) for d in range(dst)])
    fused = np.array([np.float32(float(Fraction(d + 0.5) * Fraction(scale) - Fraction(1, 2))) for d in range(dst)])
    return sep, fused


def test_where_a_contracted_fma_changes_f():
    """Finding of the sweep (src 1..399 at dst 32, 64, 96, 128, 416, 608, and the pairs of the GPU coefficient test): fused and separate
    rounding differ only where the product is an exact integer + 0.5 in double while scale is not exact -- (1, 5) at d = 2 among the GPU
    test's pairs, and (32, 96) d = 1, (32, 416) d = 6, (32, 608) d = 9 in the sweep.  There the fused f is +-2.8e-17 instead of 0: where it
    is negative, floorf gives -1 instead of 0 and the `s < 0` clamp is taken.  The GPU test runs these pairs too."""
    differing = {}
    for src, dst in COEF_PAIRS + FMA_PAIRS:
        sep, fused = _f_separate_and_fused(src, dst)
        d = np.flatnonzero(sep != fused)
        if d.size:
            differing[(src, dst)] = d.tolist()
    assert differing == {(1, 5): [2], (32, 96): [1], (32, 416): [6], (32, 608): [9]}, differing
    for (src, dst), ds in differing.items():
        sep, fused = _f_separate_and_fused(src, dst)
        assert all(sep[d] == 0.0 and 0.0 < abs(fused[d]) < 1e-12 for d in ds)


# ---- the C surface ---------------------------------------------------------------------------------------------------------------
def _decl(hdr, name):
    m = re.search(r"DT_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, "%s is not declared" % name
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    return [re.sub(r"\s*\*\s*", " *", a) for a in args]


def test_header_declares_the_entry_and_the_binding_lists_it():
    hdr = open(os.path.join(ROOT, "include", "mi355_dt.h")).read()
    assert _decl(hdr, "dt_ingest_frames") == ["dt_ctx *ctx", "const dt_frame_desc *h_desc", "int n", "uint8_t *d_dst", "int dst_h", "int dst_w"]
    for name, value in (("DT_PIX_RGB24", 0), ("DT_PIX_NV12", 1), ("DT_PIX_SWAP_RB", 16)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
        assert getattr(mi355_dt, name) == value
    m = re.search(r"typedef\s+struct\s+dt_frame_desc\s*\{(.*?)\}\s*dt_frame_desc\s*;", hdr, re.S)
    assert m, "dt_frame_desc is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["const void *d_plane0, *d_plane1", "int32_t height, width", "int32_t pitch0, pitch1", "int32_t format", "int32_t reserved"], fields
    assert [f[0] for f in mi355_dt.FrameDesc._fields_] == ["d_plane0", "d_plane1", "height", "width", "pitch0", "pitch1", "format", "reserved"]
    assert ctypes.sizeof(mi355_dt.FrameDesc) == 40
    assert "dt_ingest_frames" in mi355_dt.SYMBOLS
    assert callable(getattr(mi355_dt.Context, "ingest_frames"))
    assert re.search(r"1\.08.*?frame-ingest entry dt_ingest_frames", hdr, re.S), "the ABI comment does not say that 1.08 gained the frame-ingest entry"
    for word in ("BT.709", "I420", "10-bit", "letterboxing", "64 frames per launch"):
        assert word in hdr, "the header comment does not mention %s" % word


def test_library_exports_the_entry_and_the_abi_number_stayed():
    assert os.path.exists(mi355_dt.LIB_PATH), "libmi355_dt.so must be built in-tree (python -m object_tracking_amd.build)"
    lib = ctypes.CDLL(mi355_dt.LIB_PATH)
    assert hasattr(lib, "dt_ingest_frames"), "missing export dt_ingest_frames"
    assert lib.dt_abi_version() == 108


def test_python_surface_exists():
    from models_detection.KerasYOLO import KerasYOLO
    from models_tracking.MultiObjDetTracker import MultiObjDetTracker
    from utility import frames
    assert KerasYOLO.INGEST_SWAP_RB is False and MultiObjDetTracker.INGEST_SWAP_RB is False
    assert callable(frames.ingest_frames) and callable(frames.nv12_planes)
