"""CPU suite: the track match policy's restatement (tests/track_match_ref.py) against the track read-out restatement, the scene
worked out by hand in DESIGN.md, chunked runs, the conditions DESIGN.md states for its table, the permutation property of the
best-first order, and the declarations of the two entries.  No device; the library is not loaded."""
import os
import re

import numpy as np
import pytest

import track_match_ref as tmr
import track_readout_ref as tro

THR = 0.3
GAIN = 0.5
BEST, ANY = tmr.MATCH_BEST_FIRST, tmr.MATCH_ANY_LABEL
_REF = {}


def _case(case):
    T, cap, n_obj_t, tcap, chunkings = tmr.CASES[case]
    if case not in _REF:
        _REF[case] = tmr.moving_boxes_gt(T, cap, n_obj_t, seed=7)
    return _REF[case] + (tcap, chunkings)


def ref_of(case, match, max_age=3):
    """the restatement at gain 0.5 and min_hits 1, computed once per (case, match, max_age)"""
    key = (case, match, max_age)
    if key not in _REF:
        boxes, counts, _, tcap, _ = _case(case)
        _REF[key] = tmr.associate_tracks_match(boxes, counts, THR, max_age, GAIN, 1, match, tcap)
    return _REF[key]


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


def switches(case, match):
    _, counts, obj, _, _ = _case(case)
    return tmr.identity_switches(ref_of(case, match)["ids"], counts, obj)


# ------------------------------------------------------------------ 1. match = 0 is the read-out rule
@pytest.mark.parametrize("case", sorted(tmr.CASES))
def test_match_0_is_the_read_out_rule(case):
    boxes, counts, _, tcap, _ = _case(case)
    for a, m in ((3, 1), (0, 2)):
        want = tro.associate_tracks(boxes, counts, THR, a, GAIN, m, tcap)
        got = tro.with_min_hits(ref_of(case, 0, a), m)
        same(got, want, "max_age %d, min_hits %d" % (a, m))
        assert got["dropped"] == want["dropped"]


@pytest.mark.parametrize("case", sorted(tmr.CASES))
def test_generator_with_object_index_is_the_generator(case):
    T, cap, n_obj_t, _, _ = tmr.CASES[case]
    boxes, counts, obj, _, _ = _case(case)
    b0, c0 = tmr.moving_boxes(T, cap, n_obj_t, seed=7)
    assert np.array_equal(bits(boxes), bits(b0)) and np.array_equal(counts, c0)
    n = np.minimum(counts, cap)
    for t in range(T):
        assert (obj[t, :n[t]] >= 0).all() and (obj[t, n[t]:] == -1).all()
        assert len(set(obj[t, :n[t]].tolist())) == n[t]          # an object has one box per frame
    # without the duplicate line only the duplicated rows differ
    b1, c1, o1 = tmr.moving_boxes_gt(T, cap, n_obj_t, seed=7, duplicates=False)
    assert np.array_equal(c1, c0) and np.array_equal(o1, obj)
    diff = np.nonzero((bits(b1) != bits(b0)).any(2))
    assert set(diff[1].tolist()) <= {1} and all(t % 5 == 3 for t in diff[0].tolist())


# ------------------------------------------------------------------ 2. the worked example of DESIGN.md
def worked_example():
    boxes = np.zeros((2, 2, 8), dtype=np.float32)
    for t, xs in enumerate(((0.30, 0.40), (0.36, 0.43))):
        for i, x in enumerate(xs):
            boxes[t, i] = [x, 0.5, 0.2, 0.2, 0.9, 0, 0.8, i]
    return boxes, np.array([2, 2], dtype=np.int32)


def test_worked_example():
    boxes, counts = worked_example()
    tr = tmr.TrackMatch(2, 0.0, 0.0, 0)
    tr.frame(boxes[0, :2], 0)
    iou = tr.candidates(boxes[1, :2], 0)
    assert [round(float(iou[p]), 3) for p in ((0, 0), (0, 1), (1, 0), (1, 1))] == [0.538, 0.667, 0.212, 0.739]
    for any_label in (0, ANY):
        today = tmr.associate_tracks_match(boxes, counts, THR, 0, 0.0, 1, any_label)
        best = tmr.associate_tracks_match(boxes, counts, THR, 0, 0.0, 1, BEST | any_label)
        assert today["ids"].tolist() == [[0, 1], [1, 2]] and today["nids"] == 3
        assert best["ids"].tolist() == [[0, 1], [0, 1]] and best["nids"] == 2
        assert today["hits"].tolist() == [[1, 1], [2, 1]] and best["hits"].tolist() == [[1, 1], [2, 2]]


def test_a_label_flip_keeps_the_id_under_any_label_only():
    """one object whose label flips in frame 1: a new id without ANY_LABEL; with it the id, the hits and the velocity carry on
    and the rebuilt entry has the box's label"""
    boxes = np.zeros((3, 1, 8), dtype=np.float32)
    for t, lab in enumerate((0, 1, 1)):
        boxes[t, 0] = [0.3 + 0.01 * t, 0.5, 0.2, 0.2, 0.9, lab, 0.8, 0]
    counts = np.ones(3, dtype=np.int32)
    for best in (0, BEST):
        r = tmr.associate_tracks_match(boxes, counts, THR, 0, 1.0, 1, best)
        assert r["ids"][:, 0].tolist() == [0, 1, 1] and r["hits"][:, 0].tolist() == [1, 1, 2]
        r = tmr.associate_tracks_match(boxes, counts, THR, 0, 1.0, 1, best | ANY)
        assert r["ids"][:, 0].tolist() == [0, 0, 0] and r["hits"][:, 0].tolist() == [1, 2, 3]
        assert r["tracks"][:, 0, 4].tolist() == [0.0, 1.0, 1.0]
        assert r["tracks"][1, 0, 5] > 0                       # the velocity followed the entry of the other label


# ------------------------------------------------------------------ 3. chunked runs
@pytest.mark.parametrize("case", ["register_form", "table_over_64_then_small", "empty_frames"])
def test_chunked_runs_equal_the_whole_clip(case):
    boxes, counts, _, tcap, chunkings = _case(case)
    for match in (BEST, BEST | ANY):
        whole = ref_of(case, match)
        for chunks in chunkings:
            got = tmr.associate_tracks_match_chunked(boxes, counts, THR, 3, GAIN, 1, match, tcap, chunks)
            same(got, whole, "match %d, chunks %s" % (match, chunks))


def test_chunks_with_different_policies():
    """the policy belongs to the call: a run that switches it at the chunk boundaries equals a run of the per-frame rule with the
    switch at the same frames, and differs from every unmixed run"""
    case = "register_form_edge"
    boxes, counts, _, tcap, _ = _case(case)
    T = boxes.shape[0]
    chunks, ms = [7, 13, 11, T - 31], [0, BEST | ANY, BEST, ANY]
    got = tmr.associate_tracks_match_chunked(boxes, counts, THR, 3, GAIN, 1, ms, tcap, chunks)
    tr = tmr.TrackMatchReadout(tcap, THR, GAIN, 1)
    per_frame = [m for L, m in zip(chunks, ms) for _ in range(L)]
    ids = np.full(boxes.shape[:2], -1, dtype=np.int32)
    for t in range(T):
        tr.tm.match = per_frame[t]
        n = int(counts[t])
        ids[t, :n] = tr.frame(boxes[t, :n], 3)[0]
    assert np.array_equal(got["ids"], ids) and got["nids"] == tr.next_id
    for m in range(4):
        assert not np.array_equal(got["ids"], ref_of(case, m)["ids"]), "vacuous: the mixed run is match %d's" % m


# ------------------------------------------------------------------ 4. what DESIGN.md says of its table
def test_conditions_of_the_table():
    # the dense scene: best-first has fewer switches than today's rule
    assert switches("lds_form", BEST) < switches("lds_form", 0)
    # both flags: fewer switches than any-label alone, and fewer ids than today's rule
    assert switches("lds_form", BEST | ANY) < switches("lds_form", ANY)
    assert ref_of("lds_form", BEST | ANY)["nids"] < ref_of("lds_form", 0)["nids"]
    # the sparse scene: best-first finds today's pairs, so every output is today's
    same(ref_of("register_form", BEST), ref_of("register_form", 0), "register_form, best-first")
    # any-label mends the label flips wherever there are some
    for case in ("register_form", "register_form_edge", "lds_form", "longer_than_64_frames"):
        assert ref_of(case, ANY)["nids"] < ref_of(case, 0)["nids"] and switches(case, ANY) < switches(case, 0), case


# ------------------------------------------------------------------ 5. best-first does not depend on the order of a frame's boxes
@pytest.mark.parametrize("any_label", [0, ANY])
@pytest.mark.parametrize("scene", sorted(tmr.PERMUTATION_SCENES))
def test_best_first_is_invariant_under_a_permutation_of_the_boxes(scene, any_label):
    T, cap, n_obj, tcap = tmr.PERMUTATION_SCENES[scene]
    boxes, counts, _ = tmr.moving_boxes_gt(T, cap, lambda t: n_obj, seed=7, duplicates=False)
    shuffled = tmr.permute_frames(boxes, counts, seed=11)
    assert counts.min() >= 2 and not np.array_equal(boxes, shuffled)
    match = BEST | any_label
    a = tmr.associate_tracks_match(boxes, counts, THR, 3, GAIN, 1, match, tcap)
    b = tmr.associate_tracks_match(shuffled, counts, THR, 3, GAIN, 1, match, tcap)
    for r in (a, b):
        assert r["ties"] == 0, "an IoU tie in a row or a column: take another seed"
        assert r["dropped"] == 0
    assert a["nids"] == b["nids"]
    assert tmr.partition(a["ids"], boxes, counts) == tmr.partition(b["ids"], shuffled, counts)


def test_decode_order_is_not_invariant():
    """... and today's order does depend on it in the dense scene, which is what the property above is worth"""
    T, cap, n_obj, tcap = tmr.PERMUTATION_SCENES["general_form_dense"]
    boxes, counts, _ = tmr.moving_boxes_gt(T, cap, lambda t: n_obj, seed=7, duplicates=False)
    shuffled = tmr.permute_frames(boxes, counts, seed=11)
    a = tmr.associate_tracks_match(boxes, counts, THR, 3, GAIN, 1, 0, tcap)
    b = tmr.associate_tracks_match(shuffled, counts, THR, 3, GAIN, 1, 0, tcap)
    assert tmr.partition(a["ids"], boxes, counts) != tmr.partition(b["ids"], shuffled, counts)


# ------------------------------------------------------------------ 6. the declarations
def test_header_and_bindings_declare_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mi355_dt.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert re.search(r"dt_associate_tracks_match\(dt_ctx \*ctx, const float \*d_boxes, const int \*d_counts, int n_clips, int T, int cap, "
                     r"float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match, int \*d_ids", flat)
    assert re.search(r"dt_associate_stream_tracks_match\(dt_ctx \*ctx, const float \*d_boxes, const int \*d_counts, int n, int T, int cap, "
                     r"float thr, int max_age, float gain, int min_hits, int match, const int \*h_slots, int \*d_ids", flat)
    for name, value in (("DT_MATCH_BEST_FIRST", BEST), ("DT_MATCH_ANY_LABEL", ANY)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
    src = open(os.path.join(root, "object_tracking_amd", "mi355_dt.py")).read()
    assert '"dt_associate_tracks_match"' in src and '"dt_associate_stream_tracks_match"' in src
    assert int(re.search(r"^DT_MATCH_BEST_FIRST = (\d+)", src, re.M).group(1)) == BEST
    assert int(re.search(r"^DT_MATCH_ANY_LABEL = (\d+)", src, re.M).group(1)) == ANY
