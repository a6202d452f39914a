"""The track-memory rule's plain restatement (tests/track_memory_ref.py) checked on the CPU: it is the yardstick of
tests/test_gpu_track_memory.py, so it is held against the oracle where the oracle speaks (max_age = 0) and against a
hand-written case where it does not."""
import numpy as np
import pytest

from oracle import oracle as orc

import track_memory_ref as tm

THR = 0.3


@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_max_age_0_is_the_oracle_rule(case):
    T, cap, n_obj_t, tcap, _ = tm.CASES[case]
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    rid, rn = orc.associate_clip(boxes, counts, THR)
    ids, nids, gaps, dropped = tm.associate_memory(boxes, counts, THR, 0, tcap)
    assert np.array_equal(ids, rid) and nids == rn
    assert dropped == 0
    assert set(np.unique(gaps)) <= {-1, 0}
    assert np.array_equal(gaps == 0, (ids >= 0) & (gaps != -1))
    # and with the smallest table the rule allows: the previous frame always fits
    ids, nids, _, _ = tm.associate_memory(boxes, counts, THR, 0, cap)
    assert np.array_equal(ids, rid) and nids == rn


@pytest.mark.parametrize("case", sorted(tm.CASES))
@pytest.mark.parametrize("max_age", [1, 3, 8])
def test_chunk_invariance_and_gap_range(case, max_age):
    T, cap, n_obj_t, tcap, chunkings = tm.CASES[case]
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    ids, nids, gaps, dropped = tm.associate_memory(boxes, counts, THR, max_age, tcap)
    assert gaps.min() >= -1 and gaps.max() <= max_age
    used = np.arange(cap)[None, :] < np.minimum(counts, cap)[:, None]
    assert (ids[used] >= 0).all() and (ids[~used] == -1).all() and (gaps[~used] == -1).all()
    # every id below nids is opened exactly once, in order
    opened = ids[used & (gaps == -1)]
    assert np.array_equal(opened, np.arange(nids))
    # no id twice in one frame
    for t in range(T):
        row = ids[t, :min(counts[t], cap)]
        assert len(set(row.tolist())) == row.size
    for chunks in chunkings:
        ids2, nids2, gaps2, dropped2 = tm.associate_memory_chunked(boxes, counts, THR, max_age, tcap, chunks)
        assert np.array_equal(ids2, ids) and np.array_equal(gaps2, gaps) and nids2 == nids and dropped2 == dropped


def test_memory_bridges_gaps_on_the_stream_test_data():
    """the figures the feature was sized with: 12 objects, 40 frames, 15 % of detections dropped per frame"""
    T, cap, n_obj_t, tcap, _ = tm.CASES["register_form"]
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    n = {a: tm.associate_memory(boxes, counts, THR, a, tcap)[1] for a in (0, 1, 3)}
    assert n == {0: 119, 1: 68, 3: 55}
    gaps = tm.associate_memory(boxes, counts, THR, 3, tcap)[2]
    assert int((gaps > 0).sum()) == 64


def _frame(*rows):
    """rows (x, y, w, h, label) -> [cap = 4, 8]"""
    f = np.zeros((4, 8), dtype=np.float32)
    for i, (x, y, w, h, lab) in enumerate(rows):
        f[i] = [x, y, w, h, .9, lab, .8, i]
    return f, len(rows)


def test_hand_written_occlusion_of_two_frames():
    """A (label 0) stands still at the left and is hidden in frames 2 and 3; B (label 1) stands at the right all along; in frame
    4 a box of label 1 appears where A was (no cross-label match: a new id), in frame 5 A is back."""
    A = (.2, .5, .2, .2, 0)
    B = (.8, .5, .2, .2, 1)
    X = (.2, .5, .2, .2, 1)      # A's place, B's label
    frames = [_frame(A, B), _frame(B, A), _frame(B), _frame(B), _frame(X, B), _frame(A, B)]
    boxes = np.stack([f for f, _ in frames])
    counts = np.array([n for _, n in frames], dtype=np.int32)
    U = -1

    ids, nids, gaps, _ = tm.associate_memory(boxes, counts, THR, 3, 8)
    assert ids.tolist() == [[0, 1, U, U], [1, 0, U, U], [1, U, U, U], [1, U, U, U], [2, 1, U, U], [0, 1, U, U]]
    assert gaps.tolist() == [[U, U, U, U], [0, 0, U, U], [0, U, U, U], [0, U, U, U], [U, 0, U, U], [3, 0, U, U]]
    assert nids == 3

    # one frame of memory too few: A was last seen in frame 1, so its entry has age 3 when frame 5 looks for it
    ids, nids, gaps, _ = tm.associate_memory(boxes, counts, THR, 2, 8)
    assert ids.tolist() == [[0, 1, U, U], [1, 0, U, U], [1, U, U, U], [1, U, U, U], [2, 1, U, U], [3, 1, U, U]]
    assert gaps[5].tolist() == [U, 0, U, U] and nids == 4

    # today's rule
    ids0, n0, _, _ = tm.associate_memory(boxes, counts, THR, 0, 4)
    rid, rn = orc.associate_clip(boxes, counts, THR)
    assert np.array_equal(ids0, rid) and n0 == rn == 4

    # a table of two entries: in frame 1 it holds B and A, after frame 2 (B alone) it is [B, A aged 1] -- still two; the cut
    # bites in frame 4, whose two boxes fill the table and push A out, so A opens a new id in frame 5 -- where the two boxes
    # push out the track opened in frame 4 as well
    ids, nids, _, dropped = tm.associate_memory(boxes, counts, THR, 3, 2)
    assert ids[5].tolist() == [3, 1, U, U] and nids == 4 and dropped == 2
