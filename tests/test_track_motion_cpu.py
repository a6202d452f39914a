"""CPU suite: the track-motion rule's restatement (tests/track_motion_ref.py) against the track-memory restatement, a
hand-written occlusion, the figures DESIGN.md section 6 quotes, and chunked calls.  No device, no library."""
import numpy as np
import pytest

import track_memory_ref as tm
import track_motion_ref as tmo

THR = 0.3


def _case(case):
    T, cap, n_obj_t, tcap, chunkings = tm.CASES[case]
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    return boxes, counts, tcap, chunkings


# ------------------------------------------------------------------ 1. gain 0 is the memory rule
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_gain_0_is_the_memory_rule(case):
    boxes, counts, tcap, _ = _case(case)
    for a in (0, 1, 3):
        ref = tm.associate_memory(boxes, counts, THR, a, tcap)
        got = tmo.associate_motion(boxes, counts, THR, a, 0.0, tcap)
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], "max_age %d" % a
        assert np.array_equal(got[2], ref[2]) and got[3] == ref[3], "max_age %d" % a


# ------------------------------------------------------------------ 2. the occlusion the memory rule cannot bridge
def occluded_object():
    """one object, w = h = 0.1, x = 0.2 + 0.04 t, frames 0 .. 6, no box in frames 3 and 4"""
    T, cap = 7, 4
    boxes = np.zeros((T, cap, 8), dtype=np.float32)
    counts = np.zeros(T, dtype=np.int32)
    for t in range(T):
        if t in (3, 4):
            continue
        boxes[t, 0] = [0.2 + 0.04 * t, 0.5, 0.1, 0.1, .9, 1, .8, 0]
        counts[t] = 1
    return boxes, counts


def test_occlusion_by_hand():
    boxes, counts = occluded_object()
    ids, nids, gaps, _ = tm.associate_memory(boxes, counts, THR, 3)
    assert nids == 2 and ids[5, 0] == 1 and gaps[5, 0] == -1, "the memory rule is expected to lose the object (shift 0.12 > width 0.1)"
    for gain in (1.0, 0.5):
        ids, nids, gaps, _ = tmo.associate_motion(boxes, counts, THR, 3, gain)
        assert nids == 1, "gain %g" % gain
        assert [int(ids[t, 0]) for t in (0, 1, 2, 5, 6)] == [0] * 5
        assert int(gaps[5, 0]) == 2 and [int(gaps[t, 0]) for t in (0, 1, 2, 6)] == [-1, 0, 0, 0]
        assert (ids[3:5] == -1).all()


# ------------------------------------------------------------------ 3. the figures of the documents
TABLE = {      # case -> max_age -> (memory rule, motion gain 0.5, motion gain 1.0): ids opened, seed 7, threshold 0.3
    "register_form": {1: (68, 58, 58), 3: (55, 42, 42)},
    "register_form_edge": {1: (164, 121, 122), 3: (152, 99, 101)},
    "lds_form": {1: (226, 210, 219), 3: (214, 197, 202)},
    "longer_than_64_frames": {1: (113, 95, 95), 3: (86, 63, 63)},
}


@pytest.mark.parametrize("case", sorted(TABLE))
def test_figures_of_the_documents(case):
    boxes, counts, tcap, _ = _case(case)
    for a in (1, 3):
        mem = tm.associate_memory(boxes, counts, THR, a, tcap)[1]
        half = tmo.associate_motion(boxes, counts, THR, a, 0.5, tcap)[1]
        full = tmo.associate_motion(boxes, counts, THR, a, 1.0, tcap)[1]
        print("%s, max_age %d: ids opened -- memory %d, motion gain 0.5 %d, gain 1.0 %d" % (case, a, mem, half, full))
        if case != "lds_form":
            assert half < mem, "max_age %d: motion at gain 0.5 opens %d ids, the memory rule %d" % (a, half, mem)
        assert (mem, half, full) == TABLE[case][a], "max_age %d" % a


def test_dense_scene_caveat_at_max_age_0():
    """at max_age = 0 in dense scenes gain 1.0 can open a few MORE ids than the memory rule"""
    for case, want in (("register_form_edge", (259, 266)), ("lds_form", (290, 295))):
        boxes, counts, tcap, _ = _case(case)
        got = (tm.associate_memory(boxes, counts, THR, 0, tcap)[1], tmo.associate_motion(boxes, counts, THR, 0, 1.0, tcap)[1])
        print("%s, max_age 0: ids opened -- memory %d, motion gain 1.0 %d" % (case, got[0], got[1]))
        assert got == want


# ------------------------------------------------------------------ 4. chunked calls
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_chunked_equals_unchunked(case):
    boxes, counts, tcap, chunkings = _case(case)
    ref = tmo.associate_motion(boxes, counts, THR, 3, 0.5, tcap)
    for chunks in chunkings:
        got = tmo.associate_motion_chunked(boxes, counts, THR, 3, 0.5, tcap, chunks)
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and np.array_equal(got[2], ref[2]) and got[3] == ref[3], chunks


def test_forgetting_velocities_changes_the_result():
    """the mixing tests on the device lean on this: a plain call in the middle is visible in the ids"""
    boxes, counts, tcap, _ = _case("register_form")
    T = boxes.shape[0]
    chunks = [T // 3, T // 3, T - 2 * (T // 3)]
    mixed = tmo.associate_motion_chunked(boxes, counts, THR, 3, 0.5, tcap, chunks, plain_at=(1,))
    plain = tmo.associate_motion(boxes, counts, THR, 3, 0.5, tcap)
    assert mixed[1] != plain[1] or not np.array_equal(mixed[0], plain[0])
