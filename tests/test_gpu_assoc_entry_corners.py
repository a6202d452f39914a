"""GPU suite (-m gpu): corners of the ten dt_associate* entries that their common host path (network.hip:associate_entry) must keep.

1. A call with no clips.  dt_associate_mem and dt_associate_motion accept it before they look at T, cap or the table; the tracks
   entries look at their arguments first; every stream entry refuses n = 0.
2. A refused stream call of any level leaves the slot as it was.  The library hands out no raw view of a slot, so -- like the
   levels' own test_errors_leave_the_state_unchanged -- the slot is read back through a tracks-level continuation, whose ids depend
   on the slot's meta row (counts, next id, frame counter), whose velocities count only while vstamp equals the frame counter and
   whose hits only while hstamp does: all outputs must equal, bit for bit, those of a slot that saw no refused call.
"""
import pytest
import torch

import track_memory_ref as tm

from test_gpu_track_memory import dev, small_tracker

pytestmark = pytest.mark.gpu

THR, GAIN = 0.3, 0.5
OK, ARG = 0, 1
T, CAP, TCAP = 20, 32, 64


def _ctx():
    return small_tracker()[0].model.ctx


def _buffers(ctx, n, T, cap, tcap):
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=ctx.device)
    return dict(ids=i32(max(n, 1), max(T, 1), cap), nids=i32(max(n, 1)), gaps=i32(max(n, 1), max(T, 1), cap), hits=i32(max(n, 1), max(T, 1), cap),
                tracks=torch.full((max(n, 1), max(T, 1), tcap, 8), -7.0, device=ctx.device), tinfo=i32(max(n, 1), max(T, 1), tcap, 4),
                tcounts=i32(max(n, 1), max(T, 1)))


def raw(ctx, entry, b, c, n, T, cap, tcap=TCAP, slots=None):
    """one C entry by name on boxes b / counts c with the shape arguments as given (they need not be b's) -> return code"""
    import mi355_dt
    o = _buffers(ctx, n, T, cap, tcap)
    p = lambda k: mi355_dt._dptr(o[k])
    B, C = mi355_dt._dptr(b), mi355_dt._dptr(c)
    L, h = ctx.lib, ctx.h
    arr = ctx._slot_array(slots)[1] if slots is not None else None
    ro = (p("hits"), p("tracks"), p("tinfo"), p("tcounts"))
    ctx._sync_stream()
    if entry == "dt_associate":
        return L.dt_associate(h, B, C, n, T, cap, THR, p("ids"), p("nids"))
    if entry == "dt_associate_mem":
        return L.dt_associate_mem(h, B, C, n, T, cap, THR, 3, tcap, p("ids"), p("nids"), p("gaps"))
    if entry == "dt_associate_motion":
        return L.dt_associate_motion(h, B, C, n, T, cap, THR, 3, tcap, GAIN, p("ids"), p("nids"), p("gaps"))
    if entry == "dt_associate_tracks":
        return L.dt_associate_tracks(h, B, C, n, T, cap, THR, 3, tcap, GAIN, 2, p("ids"), p("nids"), p("gaps"), *ro)
    if entry == "dt_associate_tracks_match":
        return L.dt_associate_tracks_match(h, B, C, n, T, cap, THR, 3, tcap, GAIN, 2, 3, p("ids"), p("nids"), p("gaps"), *ro)
    if entry == "dt_associate_stream":
        return L.dt_associate_stream(h, B, C, n, T, cap, THR, arr, p("ids"), p("nids"))
    if entry == "dt_associate_stream_mem":
        return L.dt_associate_stream_mem(h, B, C, n, T, cap, THR, 3, arr, p("ids"), p("nids"), p("gaps"))
    if entry == "dt_associate_stream_motion":
        return L.dt_associate_stream_motion(h, B, C, n, T, cap, THR, 3, GAIN, arr, p("ids"), p("nids"), p("gaps"))
    if entry == "dt_associate_stream_tracks":
        return L.dt_associate_stream_tracks(h, B, C, n, T, cap, THR, 3, GAIN, 2, arr, p("ids"), p("nids"), p("gaps"), *ro)
    assert entry == "dt_associate_stream_tracks_match", entry
    return L.dt_associate_stream_tracks_match(h, B, C, n, T, cap, THR, 3, GAIN, 2, 3, arr, p("ids"), p("nids"), p("gaps"), *ro)


STREAM_ENTRIES = ("dt_associate_stream", "dt_associate_stream_mem", "dt_associate_stream_motion", "dt_associate_stream_tracks",
                  "dt_associate_stream_tracks_match")


def _scene(ctx):
    boxes, counts = tm.moving_boxes(T, CAP, lambda t: 12, seed=7)
    return (lambda a, z: dev(boxes[None, a:z], ctx)), (lambda a, z: dev(counts[None, a:z], ctx))


# ------------------------------------------------------------------ 1. no clips
@pytest.mark.parametrize("entry", ("dt_associate_mem", "dt_associate_motion"))
def test_no_clips_is_accepted_before_the_shape_is_looked_at(entry):
    ctx = _ctx()
    b, c = _scene(ctx)
    assert raw(ctx, entry, b(0, 4), c(0, 4), 0, 0, CAP) == OK
    assert raw(ctx, entry, b(0, 4), c(0, 4), 0, 4, CAP) == OK


@pytest.mark.parametrize("entry", ("dt_associate_tracks", "dt_associate_tracks_match"))
def test_no_clips_at_the_tracks_level_validates_first(entry):
    ctx = _ctx()
    b, c = _scene(ctx)
    assert raw(ctx, entry, b(0, 4), c(0, 4), 0, 0, CAP) == ARG
    assert raw(ctx, entry, b(0, 4), c(0, 4), 0, 4, CAP) == OK


@pytest.mark.parametrize("entry", STREAM_ENTRIES)
def test_no_streams_is_refused(entry):
    ctx = _ctx()
    b, c = _scene(ctx)
    ctx.stream_open(4, CAP, track_cap=TCAP)
    assert raw(ctx, entry, b(0, 4), c(0, 4), 0, 4, CAP, slots=[0]) == ARG


# ------------------------------------------------------------------ 2. a refused stream call leaves the slot alone
def test_refused_stream_calls_leave_the_slot_unchanged():
    ctx = _ctx()
    b, c = _scene(ctx)
    ctx.stream_open(4, CAP, track_cap=TCAP)
    first = {s: ctx.associate_stream_tracks(b(0, 9), c(0, 9), THR, [s], 3, GAIN, 2) for s in (1, 2)}
    for k in first[1]:
        assert torch.equal(first[1][k], first[2][k]), k
    for entry in STREAM_ENTRIES:      # slot 2: refused calls of every level -- no streams, no frames, another cap than the table's
        assert raw(ctx, entry, b(9, 20), c(9, 20), 0, 11, CAP, slots=[2]) == ARG, entry
        assert raw(ctx, entry, b(9, 20), c(9, 20), 1, 0, CAP, slots=[2]) == ARG, entry
        assert raw(ctx, entry, b(9, 20), c(9, 20), 1, 11, CAP - 1, slots=[2]) == ARG, entry
    then = {s: ctx.associate_stream_tracks(b(9, 20), c(9, 20), THR, [s], 3, GAIN, 2) for s in (1, 2, 3)}      # slot 3 is fresh
    for k in then[1]:
        assert torch.equal(then[1][k].view(torch.int32), then[2][k].view(torch.int32)), "%s differs after the refused calls" % k
    # the continuation does read what the refusals could have spoilt: a slot without the first call's table, velocities and hits gives other results
    assert not torch.equal(then[1]["ids"], then[3]["ids"])
    assert not torch.equal(then[1]["hits"], then[3]["hits"])
    assert not torch.equal(then[1]["tracks"].view(torch.int32), then[3]["tracks"].view(torch.int32))
    assert int(then[1]["hits"].max()) > 2 and bool((then[1]["tracks"][..., 5:7] != 0).any())      # hits carried over; some track moves


# The refusal the common host path makes itself, after it has looked at the stream table and before it writes the slot list: a table
# that does not fit the LDS at the call's level.  In words of LDS (160 KB = 40960): memory 14 tcap + cap, motion 18 tcap + cap, tracks
# 20 tcap + cap, tracks with BEST_FIRST 20 tcap + 4 cap.  Each table below is refused by the listed entries and taken by the level the
# slot is read back through -- the highest level that table admits, so that it reads all of the slot's state a table of that size can hold.
def _frame(ctx, b, c, s):
    i, n = ctx.associate_stream(b, c, THR, [s])
    return dict(ids=i, nids=n)


def _memory(ctx, b, c, s):
    i, n, g = ctx.associate_stream(b, c, THR, [s], max_age=3, want_gaps=True)
    return dict(ids=i, nids=n, gaps=g)


def _tracks(ctx, b, c, s):
    return ctx.associate_stream_tracks(b, c, THR, [s], 3, GAIN, 2)


LDS_REFUSALS = {
    # 14 * 3000 > 40960: no table level fits; the previous-frame rule keeps no table and runs (meta: count, next id)
    "tcap_3000": (3000, _frame, STREAM_ENTRIES[1:]),
    # 14 * 2400 + 32 fits, 18 * 2400 does not: the memory level runs (meta, ages)
    "tcap_2400": (2400, _memory, STREAM_ENTRIES[2:]),
    # 20 * 2044 + 32 = 40912 fits, 20 * 2044 + 4 * 32 = 41008 does not: the tracks level runs (meta, vstamp, hstamp), BEST_FIRST is refused
    "tcap_2044": (2044, _tracks, STREAM_ENTRIES[4:]),
}


@pytest.mark.parametrize("case", sorted(LDS_REFUSALS))
def test_lds_refusals_on_a_stream_leave_the_slot_unchanged(case):
    tcap, call, refused = LDS_REFUSALS[case]
    ctx = _ctx()
    b, c = _scene(ctx)
    ctx.stream_open(4, CAP, track_cap=tcap)
    for s in (1, 2):
        call(ctx, b(0, 9), c(0, 9), s)
    for entry in refused:
        assert raw(ctx, entry, b(9, 20), c(9, 20), 1, 11, CAP, tcap=tcap, slots=[2]) == ARG, entry
    then = {s: call(ctx, b(9, 20), c(9, 20), s) for s in (1, 2, 3)}      # slot 3 is fresh
    for k in then[1]:
        assert torch.equal(then[1][k].view(torch.int32), then[2][k].view(torch.int32)), "%s differs after the refused calls" % k
    assert not torch.equal(then[1]["ids"], then[3]["ids"])
