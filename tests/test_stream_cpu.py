"""Stream slots, the parts that need no GPU: the key -> slot bookkeeping (models_tracking/streams.py) and the C surface
as the header declares it."""
import os
import re

import pytest

import mi355_dt
from models_tracking.streams import StreamTable, StreamTableError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeTracker(object):
    def __init__(self):
        self.calls = []

    def open_streams(self, n_slots, cap=None):
        self.calls.append(("open", n_slots, cap))

    def reset_streams(self, slots=None):
        self.calls.append(("reset", list(slots)))


def test_stream_table_opens_the_device_table_and_hands_out_slots():
    trk = FakeTracker()
    t = StreamTable(trk, n_slots=3, cap=40)
    assert trk.calls == [("open", 3, 40)]
    assert [t.open(k) for k in ("cam-a", "cam-b", "cam-c")] == [0, 1, 2]
    assert len(t) == 3 and "cam-b" in t and "cam-x" not in t
    assert t.slots(["cam-c", "cam-a"]) == [2, 0]
    assert t.keys() == ["cam-a", "cam-b", "cam-c"]


def test_stream_table_release_resets_and_the_slot_is_reused():
    trk = FakeTracker()
    t = StreamTable(trk, n_slots=3)
    for k in ("a", "b", "c"):
        t.open(k)
    assert t.release("b") == 1
    assert trk.calls[-1] == ("reset", [1])
    assert "b" not in t and len(t) == 2
    assert t.open("d") == 1                     # the released slot, not a new one
    t.release("a"); t.release("c")
    assert [t.open("e"), t.open("f")] == [0, 2]   # lowest free number first
    assert [c for c in trk.calls if c[0] == "reset"] == [("reset", [1]), ("reset", [0]), ("reset", [2])]


def test_stream_table_full_unknown_and_duplicate_keys_are_clear_errors():
    t = StreamTable(None, n_slots=2)
    t.open("a"); t.open("b")
    with pytest.raises(StreamTableError) as e:
        t.open("c")
    assert "no free slot" in str(e.value) and "'c'" in str(e.value) and "2" in str(e.value)
    with pytest.raises(StreamTableError) as e:
        t.slot("nope")
    assert "unknown stream 'nope'" in str(e.value)
    with pytest.raises(StreamTableError) as e:
        t.release("nope")
    assert "unknown stream" in str(e.value)
    with pytest.raises(StreamTableError) as e:
        t.open("a")
    assert "already open" in str(e.value)
    with pytest.raises(StreamTableError):
        t.slots(["a", "a"])
    assert isinstance(e.value, KeyError)
    with pytest.raises(ValueError):
        StreamTable(None, n_slots=0)
    assert t.slots(["b", "a"]) == [1, 0]        # the failures changed nothing


def _decl(hdr, name):
    m = re.search(r"DT_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, "%s is not declared" % name
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    return [re.sub(r"\s*\*\s*", " *", a) for a in args]


def test_header_declares_the_stream_entries_and_the_binding_lists_them():
    hdr = open(os.path.join(ROOT, "include", "mi355_dt.h")).read()
    assert _decl(hdr, "dt_stream_open") == ["dt_ctx *ctx", "int n_slots", "int cap"]
    assert _decl(hdr, "dt_stream_reset") == ["dt_ctx *ctx", "const int *h_slots", "int n"]
    assert _decl(hdr, "dt_track_stream_forward") == ["dt_ctx *ctx", "const void *d_frames", "int frames_dtype", "int n", "int T",
                                                     "const int *h_slots", "float *d_trk", "float *d_det"]
    assert _decl(hdr, "dt_associate_stream") == ["dt_ctx *ctx", "const float *d_boxes", "const int *d_counts", "int n", "int T", "int cap",
                                                 "float thr", "const int *h_slots", "int *d_ids", "int *d_nids"]
    for s in ("dt_stream_open", "dt_stream_reset", "dt_track_stream_forward", "dt_associate_stream"):
        assert s in mi355_dt.SYMBOLS
    for meth in ("stream_open", "stream_reset", "track_stream_forward", "associate_stream"):
        assert callable(getattr(mi355_dt.Context, meth))
    assert re.search(r"1\.08[^\n]*stream", hdr), "the ABI comment does not say that 1.08 gained the stream entries"
