"""Tiny-tracker streams, the parts that need no GPU: the C surface as the header declares it, the Python surface, the
key -> slot bookkeeping driving a tiny tracker, and what "carried state" means (tests/tiny_stream_ref.py against the oracle)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mi355_dt
from models_tracking.streams import StreamTable
from oracle import oracle as orc
from utility import synth

import tiny_stream_ref as tsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dt_tiny_stream_open", "dt_tiny_stream_reset", "dt_tiny_stream_sequence", "dt_tiny_stream_forward")


def _decl(hdr, name):
    m = re.search(r"DT_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, "%s is not declared" % name
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    return [re.sub(r"\s*\*\s*", " *", a) for a in args]


def test_header_declares_the_tiny_stream_entries():
    hdr = open(os.path.join(ROOT, "include", "mi355_dt.h")).read()
    assert _decl(hdr, "dt_tiny_stream_open") == ["dt_ctx *ctx", "int n_slots"]
    assert _decl(hdr, "dt_tiny_stream_reset") == ["dt_ctx *ctx", "const int *h_slots", "int n"]
    assert _decl(hdr, "dt_tiny_stream_sequence") == ["dt_ctx *ctx", "const float *d_x", "int n", "int T", "const int *h_slots", "float *d_out"]
    assert _decl(hdr, "dt_tiny_stream_forward") == ["dt_ctx *ctx", "const float *d_feat", "const float *d_det", "int n", "int T", "int fh", "int fw",
                                                    "int fc", "int pool", "const int *h_slots", "float *d_out"]
    assert re.search(r"1\.08[^/]*dt_tiny_stream_open", hdr), "the ABI comment does not say that 1.08 gained the tiny stream entries"


def test_binding_lists_them_and_the_library_exports_them():
    for s in ENTRIES:
        assert s in mi355_dt.SYMBOLS
    assert os.path.exists(mi355_dt.LIB_PATH), "libmi355_dt.so must be built in-tree (python -m object_tracking_amd.build)"
    lib = ctypes.CDLL(mi355_dt.LIB_PATH)
    for s in ENTRIES:
        assert hasattr(lib, s), "missing export " + s
    assert lib.dt_abi_version() == 108


def test_python_surface_exists():
    from models_tracking.TinyHeatmapTracker import TinyHeatmapTracker
    from models_tracking.TinyTracker import TinyTracker
    for meth in ("tiny_stream_open", "tiny_stream_reset", "tiny_stream_sequence", "tiny_stream_forward"):
        assert callable(getattr(mi355_dt.Context, meth))
    for cls in (TinyTracker, TinyHeatmapTracker):
        for meth in ("open_streams", "reset_streams", "track_stream"):
            assert callable(getattr(cls, meth)), (cls.__name__, meth)
    assert TinyHeatmapTracker.track_stream is not TinyTracker.track_stream      # (heat, rects), not boxes
    assert "ignored" in TinyTracker.open_streams.__doc__ and "cap" in TinyTracker.open_streams.__doc__


class FakeCtx(object):
    def __init__(self):
        self.calls = []

    def tiny_stream_open(self, n_slots):
        self.calls.append(("open", n_slots))

    def tiny_stream_reset(self, slots=None):
        self.calls.append(("reset", None if slots is None else list(slots)))


def fake_tiny_tracker():
    """a TinyTracker whose context records the calls: its own open_streams / reset_streams run"""
    from models_tracking.TinyTracker import TinyTracker
    tt = TinyTracker.__new__(TinyTracker)

    class Model(object):
        ctx = FakeCtx()
    tt.model_tracker = Model()
    return tt, Model.ctx


def test_stream_table_drives_a_tiny_tracker():
    tt, ctx = fake_tiny_tracker()
    t = StreamTable(tt, n_slots=3, cap=40)            # cap travels to open_streams and stops there
    assert ctx.calls == [("open", 3)]
    assert [t.open(k) for k in ("obj-a", "obj-b", "obj-c")] == [0, 1, 2]
    assert t.release("obj-b") == 1
    assert ctx.calls[-1] == ("reset", [1])            # release, then reset
    assert t.open("obj-d") == 1                       # the released slot, not a new one
    t.release("obj-a"); t.release("obj-c")
    assert [t.open("e"), t.open("f")] == [0, 2]       # lowest free number first
    assert [c for c in ctx.calls if c[0] == "reset"] == [("reset", [1]), ("reset", [0]), ("reset", [2])]
    tt.reset_streams()
    assert ctx.calls[-1] == ("reset", None)


@pytest.mark.parametrize("pool,fh,fw,fc", [("Global", 4, 4, 32), ("Max", 8, 8, 32)])
def test_chunked_reference_equals_the_oracle_on_the_concatenation(pool, fh, fw, fc):
    """carried h and c, chunk by chunk, are the oracle's recurrence bit for bit -- whatever the chunking, with streams out of step,
    and a reset slot starts again"""
    feat_dim = fc if pool == "Global" else (fh // 4) * (fw // 4) * fc
    tw = synth.synth_tiny_weights(feat_dim)
    rs = np.random.RandomState(5)
    n, T = 3, 9
    feat = rs.randn(n, T, fh, fw, fc).astype(np.float32)
    det = rs.rand(n, T, 4).astype(np.float32)
    whole = orc.tinytracker_forward(feat, det, tw, pool=pool)
    for chunks in ([9], [1] * 9, [2, 3, 4], [4, 5]):
        got = tsr.run_chunks(tsr.TinyStreams(tw, pool), feat, det, chunks, [4, 0, 2])
        assert np.array_equal(got, whole), chunks
    # out of step: stream 0 alone for two frames, then all three, then a reset of one
    s = tsr.TinyStreams(tw, pool)
    a = s.forward(feat[:1, :2], det[:1, :2], [7])
    b = s.forward(np.concatenate([feat[:1, 2:5], feat[1:, :3]]), np.concatenate([det[:1, 2:5], det[1:, :3]]), [7, 1, 3])
    assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0, :5])
    assert np.array_equal(b[1:], whole[1:, :3])
    s.reset([1])
    c = s.forward(feat[1:, :3], det[1:, :3], [1, 3])
    assert np.array_equal(c[0], whole[1, :3]) and not np.array_equal(c[1], whole[2, :3])
