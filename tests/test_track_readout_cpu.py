"""CPU suite: the track read-out's restatement (tests/track_readout_ref.py) against the track-motion restatement, a scene
worked out by hand, chunked calls, the conditions that keep the device tests from being vacuous, and the declarations of the two
entries.  No device; the library is not loaded."""
import os
import re

import numpy as np
import pytest

import track_memory_ref as tm
import track_motion_ref as tmo
import track_readout_ref as tro

THR = 0.3
GAIN = 0.5
_REF = {}


def _case(case):
    T, cap, n_obj_t, tcap, chunkings = tm.CASES[case]
    if case not in _REF:
        _REF[case] = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    return _REF[case] + (tcap, chunkings)


def ref_of(case, max_age, min_hits=1):
    """the restatement at gain 0.5, computed once per (case, max_age): min_hits filters the read-out only"""
    key = (case, max_age)
    if key not in _REF:
        boxes, counts, tcap, _ = _case(case)
        _REF[key] = tro.associate_tracks(boxes, counts, THR, max_age, GAIN, 1, tcap)
    return tro.with_min_hits(_REF[key], min_hits)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same(got, ref, what=""):
    for k in tro.KEYS:
        if k == "nids":
            assert got[k] == ref[k], "%s: nids" % what
        elif k == "tracks":
            assert np.array_equal(bits(got[k]), bits(ref[k])), "%s: tracks (bits)" % what
        else:
            assert np.array_equal(got[k], ref[k]), "%s: %s" % (what, k)


# ------------------------------------------------------------------ 1. the match is the motion rule's
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_ids_are_the_motion_rules(case):
    boxes, counts, tcap, _ = _case(case)
    for a in (0, 1, 3):
        want = tmo.associate_motion(boxes, counts, THR, a, GAIN, tcap)
        for m in (1, 3):
            got = tro.associate_tracks(boxes, counts, THR, a, GAIN, m, tcap) if (a, m) == (3, 3) else ref_of(case, a, m)
            assert np.array_equal(got["ids"], want[0]) and got["nids"] == want[1], "max_age %d, min_hits %d" % (a, m)
            assert np.array_equal(got["gaps"], want[2]) and got["dropped"] == want[3], "max_age %d, min_hits %d" % (a, m)
            # with_min_hits is the shortcut the other tests take: once per case it is checked against a run of its own
            if (a, m) == (3, 3):
                same(got, ref_of(case, a, m), "min_hits filters the read-out only")
            # hits of a box: 1 for a new id, otherwise one more than the track's last
            assert ((got["hits"] == 1) == ((got["gaps"] == -1) & (got["ids"] >= 0))).all()
            assert ((got["hits"] == -1) == (got["ids"] == -1)).all()


# ------------------------------------------------------------------ 2. a scene worked out by hand
def occluded_object_and_ghost():
    """one object, w = h = 0.25, y = 0.5, x = 0.25 + t/16 (every number a binary fraction: the arithmetic below is exact),
    frames 0 .. 6, no box in frames 3 and 4; in frame 1 a ghost box of the same label, far away, in FRONT of the object in decode order"""
    T, cap = 7, 4
    boxes = np.zeros((T, cap, 8), dtype=np.float32)
    counts = np.zeros(T, dtype=np.int32)
    for t in range(T):
        if t in (3, 4):
            continue
        obj = [0.25 + t / 16.0, 0.5, 0.25, 0.25, .9, 1, .8, 0]
        if t == 1:
            boxes[t, 0] = [0.875, 0.125, 0.125, 0.125, .7, 1, .6, 0]
            boxes[t, 1] = obj
            counts[t] = 2
        else:
            boxes[t, 0] = obj
            counts[t] = 1
    return boxes, counts


def test_scene_by_hand():
    boxes, counts = occluded_object_and_ghost()
    r = tro.associate_tracks(boxes, counts, THR, 3, 1.0, 2)
    # the object is id 0 throughout, the ghost id 1; gain 1 makes the velocity 1/16 per frame from frame 1 on
    assert r["nids"] == 2
    assert [int(r["ids"][t, 0]) for t in (0, 2, 5, 6)] == [0] * 4 and r["ids"][1, :2].tolist() == [1, 0]
    assert int(r["gaps"][5, 0]) == 2
    assert [int(r["hits"][t, 0]) for t in (0, 2, 5, 6)] == [1, 3, 4, 5] and r["hits"][1, :2].tolist() == [1, 2]
    # frame 0: the object has one hit, not confirmed.  From frame 1 on exactly one row, the object's: the ghost (one hit) coasts in
    # the table through frames 2 .. 4 and is never read out
    assert r["track_counts"].tolist() == [0, 1, 1, 1, 1, 1, 1]
    v = 1.0 / 16.0
    want = {      # t -> (x, (id, age, hits, box))
        1: (0.25 + 1 * v, (0, 0, 2, 1)),          # box 1 of the frame: the ghost is box 0
        2: (0.25 + 2 * v, (0, 0, 3, 0)),
        3: (0.25 + 2 * v + 1 * v, (0, 1, 3, -1)),      # coasting: last seen at 0.375, one and two steps on
        4: (0.25 + 2 * v + 2 * v, (0, 2, 3, -1)),
        5: (0.25 + 5 * v, (0, 0, 4, 0)),          # returns with its id where the third step predicted it
        6: (0.25 + 6 * v, (0, 0, 5, 0)),
    }
    for t, (x, info) in want.items():
        assert r["tracks"][t, 0].tolist() == [x, 0.5, 0.25, 0.25, 1.0, v, 0.0, 0.0], t
        assert tuple(r["track_info"][t, 0]) == info, t
        assert (r["tracks"][t, 1:] == 0).all() and (r["track_info"][t, 1:] == -1).all()
    assert (r["tracks"][0] == 0).all() and (r["track_info"][0] == -1).all()
    assert not (r["track_info"][..., 0] == 1).any(), "the ghost was read out"
    # min_hits = 1 shows the ghost: in frame 1, and coasting at rest through frames 2 .. 4 (max_age 3)
    r1 = tro.with_min_hits(r, 1)
    assert r1["track_counts"].tolist() == [1, 2, 2, 2, 2, 1, 1]
    assert [tuple(r1["track_info"][t, 1]) for t in (2, 3, 4)] == [(1, 1, 1, -1), (1, 2, 1, -1), (1, 3, 1, -1)]
    assert all(r1["tracks"][t, 1].tolist() == [0.875, 0.125, 0.125, 0.125, 1.0, 0.0, 0.0, 0.0] for t in (2, 3, 4))


def test_age_0_rows_keep_the_sign_of_zero():
    """an entry of age 0 reports its stored bits: x = -0.0 stays -0.0 (x + 0 * vx would give +0.0)"""
    boxes = np.zeros((2, 2, 8), dtype=np.float32)
    boxes[:, 0] = [-0.0, 0.5, 0.25, 0.25, .9, 1, .8, 0]
    counts = np.ones(2, dtype=np.int32)
    r = tro.associate_tracks(boxes, counts, THR, 1, 1.0, 1)
    assert r["ids"][:, 0].tolist() == [0, 0]
    assert bits(r["tracks"][:, 0, 0]).tolist() == [np.int32(-2 ** 31)] * 2


# ------------------------------------------------------------------ 3. chunked calls
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_chunked_equals_unchunked(case):
    boxes, counts, tcap, chunkings = _case(case)
    ref = ref_of(case, 3, 3)
    for chunks in chunkings:
        got = tro.associate_tracks_chunked(boxes, counts, THR, 3, GAIN, 3, tcap, chunks)
        same(got, ref, "chunks %s" % chunks)
        assert got["dropped"] == ref["dropped"]


def test_a_middle_chunk_that_forgets_the_hits():
    """a middle chunk through dt_associate_stream_motion: the match is unchanged, every track starts counting again"""
    boxes, counts, tcap, _ = _case("register_form")
    T = boxes.shape[0]
    third = T // 3
    chunks = [third, third, T - 2 * third]
    ref = ref_of("register_form", 3, 3)
    got = tro.associate_tracks_chunked(boxes, counts, THR, 3, GAIN, 3, tcap, chunks, motion_at=(1,))
    for k in ("ids", "gaps"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["nids"] == ref["nids"]
    a, z = third, 2 * third
    for k in ("hits", "tracks", "track_info", "track_counts"):
        assert np.array_equal(got[k][:a], ref[k][:a]), k
    assert (got["hits"][a:z] == -1).all() and (got["track_counts"][a:z] == 0).all()
    # after the chunk: the first frame's hits are 1 or 2, so nothing is confirmed at min_hits = 3 until the frame after
    assert got["hits"][z].max() == 2 and got["track_counts"][z] == 0 and ref["track_counts"][z] > 0
    assert not np.array_equal(got["hits"][z:], ref["hits"][z:])
    # a middle chunk through the memory entry forgets the velocities too: that one changes the ids
    mixed = tro.associate_tracks_chunked(boxes, counts, THR, 3, GAIN, 3, tcap, chunks, plain_at=(1,))
    want = tmo.associate_motion_chunked(boxes, counts, THR, 3, GAIN, tcap, chunks, plain_at=(1,))
    assert np.array_equal(mixed["ids"], want[0]) and mixed["nids"] == want[1] and np.array_equal(mixed["gaps"], want[2])
    assert not np.array_equal(mixed["ids"], ref["ids"])


# ------------------------------------------------------------------ 4. the device tests are not vacuous
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_non_vacuity(case):
    boxes, counts, tcap, _ = _case(case)
    cap = boxes.shape[1]
    rows = {}
    for a in (0, 1, 3):
        for m in (1, 3):
            r = ref_of(case, a, m)
            n = int(r["track_counts"].sum())
            coasting = r["track_info"][..., 3] == -1
            coasting &= r["track_info"][..., 0] >= 0
            rows[a, m] = (n, int(coasting.sum()))
            if m == 3:
                vel = r["tracks"][..., 5:7][coasting]
                assert (vel != 0).any(axis=1).all(), "max_age %d: a confirmed coasting row at rest" % a
    print("%s: boxes %d; (max_age, min_hits) -> (rows, coasting rows) %s" % (case, int(np.minimum(counts, cap).sum()), rows))
    for a in (1, 3):
        assert rows[a, 1][1] > 0 and rows[a, 3][1] > 0, "max_age %d: no coasting rows" % a
    assert rows[0, 1] == (int(np.minimum(counts, cap).sum()), 0), "max_age 0, min_hits 1: the read-out is the boxes"
    for a in (0, 1, 3):
        assert 0 < rows[a, 3][0] < rows[a, 1][0], "max_age %d: min_hits 3 removes no row, or all" % a


# ------------------------------------------------------------------ 5. the entries are declared and bound
def test_header_and_bindings_have_the_entries():
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "mi355_dt.h")).read()
    for name in ("dt_associate_tracks", "dt_associate_stream_tracks"):
        assert re.search(r"DT_API\s+int\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+DT_TRACK_FLOATS\s+8\b", header) and re.search(r"#define\s+DT_TRACK_INTS\s+4\b", header)
    import mi355_dt
    assert "dt_associate_tracks" in mi355_dt.SYMBOLS and "dt_associate_stream_tracks" in mi355_dt.SYMBOLS
    assert (mi355_dt.DT_TRACK_FLOATS, mi355_dt.DT_TRACK_INTS) == (tro.TRACK_FLOATS, tro.TRACK_INTS)
    for name in ("associate_tracks", "associate_stream_tracks"):
        assert callable(getattr(mi355_dt.Context, name, None)), name
    from models_tracking.MultiObjDetTracker import MultiObjDetTracker
    assert MultiObjDetTracker.MIN_HITS is None and callable(MultiObjDetTracker.tracks_from_result)
