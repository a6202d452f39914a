"""Track scores: the restatement tests/track_scored_ref.py against the restatements it builds on, the
properties the two-pass match must have, and the declarations.  No device.
"""
import os
import re

import numpy as np
import pytest

import track_assign_ref as tar
import track_scored_ref as tsr

THR, GAIN = tsr.THR, tsr.GAIN
BEST, ANY = tsr.MATCH_BEST_FIRST, tsr.MATCH_ANY_LABEL
SCENES = sorted(tsr.SCENES)
KEYS = tsr.KEYS


def equal(a, b, what=""):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (what, key)


# ------------------------------------------------------------------ 1. the scenes are not vacuous
@pytest.mark.parametrize("match", [0, ANY])
@pytest.mark.parametrize("name", SCENES)
def test_scenes_are_not_vacuous(name, match):
    """floors well inside what the recipe gives (27 .. 236 pairs of the second pass, 64 .. 286 dropped boxes, 121 .. 604 pairs whose
    entry was dead -- each such pair counted once per frame; the floor of 100 holds under ANY_LABEL too), so that the device tests
    cannot pass on scenes where nothing happens"""
    T, cap, _, tcap, max_age, _, _, _ = tsr.SCENES[name]
    r = tsr.scene_ref(name, match)
    s = r["stats"]
    print(name, match, s, "ids opened", r["nids"])
    assert s["pass2"] >= 20 and s["dropped_boxes"] >= 50 and s["dead_candidates"] >= 100 and s["pass1"] >= 100
    assert r["dropped"] == 0, "a capacity cut"
    boxes, counts = tsr.scene(name)
    used = np.arange(cap)[None, :] < counts[:, None]
    assert int(((r["ids"] == -1) & used).sum()) == s["dropped_boxes"] == int((r["hits"] == 0).sum())
    assert ((r["hits"] == -1) == ~used).all() and (r["gaps"][r["ids"] == -1] == -1).all()
    plain = tar.associate_tracks_assign(boxes, counts, THR, max_age, GAIN, 1, match, tcap)
    assert all(not np.array_equal(r["ids"][t], plain["ids"][t]) for t in range(T)), "some frame is the plain assignment's"
    assert r["nids"] < plain["nids"]
    # no read-out row is a dead one, and an age-0 row's box is the box that carries its id
    for t in range(T):
        for k in range(int(r["track_counts"][t])):
            tid, age, hits, box = r["track_info"][t, k]
            assert tid >= 0 and hits >= 1
            if age == 0:
                assert r["ids"][t, box] == tid


def test_ids_opened_are_the_issues():
    """the four scenes at match 0: the two-pass rule against the plain assignment on all boxes"""
    got = [tsr.scene_ref(name, 0)["nids"] for name in ("crowd_reg_grow", "crowd_reg", "crowd_lds", "crowd_long")]
    assert got == [34, 26, 75, 85]


# ------------------------------------------------------------------ 2. the equivalences
@pytest.mark.parametrize("match", [0, ANY])
@pytest.mark.parametrize("name", SCENES)
def test_all_boxes_confident_is_the_plain_assignment(name, match):
    T, cap, _, tcap, max_age, _, _, _ = tsr.SCENES[name]
    boxes, counts = tsr.scene(name)
    got = tsr.associate_tracks_scored(boxes, counts, THR, max_age, GAIN, 2, match, tcap, score_high=0.0, score_new=0.0)
    assert got["stats"]["pass2"] == 0 and got["stats"]["dropped_boxes"] == 0 and got["stats"]["dead_candidates"] == 0
    equal(got, tar.associate_tracks_assign(boxes, counts, THR, max_age, GAIN, 2, match, tcap), name)


@pytest.mark.parametrize("name", SCENES)
def test_without_the_second_pass_the_weak_boxes_are_not_there(name):
    T, cap, _, tcap, max_age, _, match, _ = tsr.SCENES[name]
    boxes, counts = tsr.scene(name)
    got = tsr.associate_tracks_scored(boxes, counts, THR, max_age, GAIN, 1, match, tcap, score_new=tsr.SCORE_HIGH, max_age_low=-1)
    hb, hc, index = tsr.compact_high(boxes, counts, tsr.SCORE_HIGH)
    want = tar.associate_tracks_assign(hb, hc, THR, max_age, GAIN, 1, match, tcap)
    assert got["dropped"] == 0 and want["dropped"] == 0
    assert got["stats"]["pass2"] == 0 and got["nids"] == want["nids"] and 0 < int(hc.sum()) < int(counts.sum())
    for t in range(T):
        for i in range(int(counts[t])):
            k = index[t, i]
            if k < 0:
                assert (got["ids"][t, i], got["gaps"][t, i], got["hits"][t, i]) == (-1, -1, 0)
            else:
                assert (got["ids"][t, i], got["gaps"][t, i], got["hits"][t, i]) == (want["ids"][t, k], want["gaps"][t, k], want["hits"][t, k])


# ------------------------------------------------------------------ 3. the smallest case
def test_worked_example():
    """a track's box turns weak for one frame beside a weak clutter box: the track goes on, the clutter opens nothing"""
    boxes, counts = tsr.worked_example()
    for tcap in (2, 80):
        r = tsr.associate_tracks_scored(boxes, counts, 0.3, 0, 0.5, 1, 0, tcap)
        assert r["ids"].tolist() == [[0, -1], [-1, 0], [0, -1]] and r["nids"] == 1
        assert r["hits"].tolist() == [[1, -1], [0, 2], [3, -1]]
        assert r["gaps"].tolist() == [[-1, -1], [-1, 0], [0, -1]]
        assert r["stats"] == dict(pass1=1, pass2=1, dropped_boxes=1, dead_candidates=0)
        plain = tar.associate_tracks_assign(boxes, counts, 0.3, 0, 0.5, 1, 0, tcap)
        assert plain["nids"] == 2
        hb, hc, _ = tsr.compact_high(boxes, counts, tsr.SCORE_HIGH)
        assert hc.tolist() == [1, 0, 1] and tar.associate_tracks_assign(hb, hc, 0.3, 0, 0.5, 1, 0, tcap)["nids"] == 2


# ------------------------------------------------------------------ 4. every parameter matters
def test_parameters_change_the_result():
    base = tsr.scene_ref("crowd_reg", 0)
    assert tsr.SCENES["crowd_reg"][4] == 2
    assert not np.array_equal(tsr.scene_ref("crowd_reg", 0, max_age_low=2)["ids"], base["ids"])
    assert not np.array_equal(tsr.scene_ref("crowd_reg", 0, thr_low=0.5)["ids"], base["ids"])
    boxes, counts = tsr.scene("crowd_reg")
    _, _, _, tcap, max_age, _, _, _ = tsr.SCENES["crowd_reg"]
    swapped = tsr.associate_tracks_scored(tsr.swap_floats(boxes, 4, 6), counts, THR, max_age, GAIN, 1, 0, tcap, score_at=4)
    for key in ("ids", "nids", "gaps", "hits", "track_info", "track_counts"):      # (the boxes themselves are no output)
        assert np.array_equal(swapped[key], base[key]), key
    other = tsr.associate_tracks_scored(boxes, counts, THR, max_age, GAIN, 1, 0, tcap, score_at=4)      # float 4 = score + .05
    assert not np.array_equal(other["ids"], base["ids"])


def test_a_nan_score_is_low():
    boxes, counts = tsr.worked_example()
    boxes = boxes.copy()
    boxes[2, 0, 6] = np.nan
    r = tsr.associate_tracks_scored(boxes, counts, 0.3, 0, 0.5, 1, 0, 2)
    assert r["ids"].tolist() == [[0, -1], [-1, 0], [0, -1]] and r["stats"]["pass2"] == 2      # matched, in the second pass
    boxes[0, 0, 6] = np.nan
    assert tsr.associate_tracks_scored(boxes, counts, 0.3, 0, 0.5, 1, 0, 2)["nids"] == 0         # ... and opens nothing


# ------------------------------------------------------------------ 5. chunks
CHUNKS = {"crowd_reg_grow": [1, 4, 7], "crowd_reg": [1, 4, 7], "crowd_lds": [2, 1, 3], "crowd_long": [30, 36]}


@pytest.mark.parametrize("name", SCENES)
def test_chunked_runs_equal_the_whole_clip(name):
    T, cap, _, tcap, max_age, _, match, _ = tsr.SCENES[name]
    boxes, counts = tsr.scene(name)
    assert sum(CHUNKS[name]) == T
    got = tsr.associate_tracks_scored_chunked(boxes, counts, THR, max_age, GAIN, 2, match, tcap, CHUNKS[name])
    equal(got, tsr.scene_ref(name, match, min_hits=2), name)
    assert got["stats"] == tsr.scene_ref(name, match)["stats"]


@pytest.mark.parametrize("name", ["crowd_reg", "crowd_lds"])
def test_chunks_through_other_entries_meet_dead_rows(name):
    """the middle chunk stands for another entry: it finds the dead rows of the scored chunk before it, would match them, and must not"""
    T, cap, _, tcap, max_age, _, _, _ = tsr.SCENES[name]
    boxes, counts = tsr.scene(name)
    chunks = [T // 3, T // 3, T - 2 * (T // 3)]
    whole = tsr.scene_ref(name, 0)
    for kw in (dict(assign_at=(1,)), dict(match_at={1: BEST}), dict(motion_at=(1,))):
        tr = tsr.TrackScoredReadout(tcap, THR, GAIN, 1, 0)
        tr.clip(boxes[:chunks[0]], counts[:chunks[0]], max_age)
        before = tr.tm.stats["dead_candidates"]
        assert any(e[2] < 0 for e in tr.tm.table), "vacuous: the first chunk leaves no dead row"
        tr.tm.scored = False
        tr.tm.assign = "assign_at" in kw
        tr.tm.match = BEST if "match_at" in kw else 0
        tr.frame(boxes[chunks[0], :counts[chunks[0]]], max_age)
        assert tr.tm.stats["dead_candidates"] > before, "vacuous: no box of the next frame overlaps a dead row"
        assert all(e[2] >= 0 for e in tr.tm.table), "a dead row survived a rebuild"
        mixed = tsr.associate_tracks_scored_chunked(boxes, counts, THR, max_age, GAIN, 1, 0, tcap, chunks, **kw)
        assert not np.array_equal(mixed["ids"], whole["ids"])
        assert int(((mixed["ids"][chunks[0]:2 * chunks[0]] == -1) & (mixed["gaps"][chunks[0]:2 * chunks[0]] == -1)).sum()) == \
            int((np.arange(cap)[None, :] >= counts[chunks[0]:2 * chunks[0], None]).sum()), "another entry dropped a box"


# ------------------------------------------------------------------ 6. the declarations
def test_header_and_bindings_declare_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mi355_dt.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert re.search(r"dt_associate_tracks_scored\(dt_ctx \*ctx, const float \*d_boxes, const int \*d_counts, int n_clips, int T, int cap, "
                     r"float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match, int score_at, float score_high, "
                     r"float score_new, float assoc_threshold_low, int max_age_low, int \*d_ids, int \*d_nids, int \*d_gaps, int \*d_hits, "
                     r"float \*d_tracks, int \*d_tinfo, int \*d_tcounts\)", flat)
    assert re.search(r"dt_associate_stream_tracks_scored\(dt_ctx \*ctx, const float \*d_boxes, const int \*d_counts, int n, int T, int cap, "
                     r"float thr, int max_age, float gain, int min_hits, int match, int score_at, float score_high, float score_new, "
                     r"float thr_low, int max_age_low, const int \*h_slots, int \*d_ids, int \*d_nids, int \*d_gaps, int \*d_hits, "
                     r"float \*d_tracks, int \*d_tinfo, int \*d_tcounts\)", flat)
    text = re.sub(r"\s+", " ", re.sub(r"\n \* ", " ", header))      # the comments without their line starts
    for phrase in ("26 * tcap + 5 * cap + 6 words must not exceed 40960", "never survives the next rebuild", "DOES count in the capacity cut",
                   "Not done here: a Kalman filter"):
        assert phrase in text, phrase
    src = open(os.path.join(root, "object_tracking_amd", "mi355_dt.py")).read()
    assert '"dt_associate_tracks_scored"' in src and '"dt_associate_stream_tracks_scored"' in src
    trk = open(os.path.join(root, "object_tracking_amd", "models_tracking", "MultiObjDetTracker.py")).read()
    for line in ("SCORE_HIGH = None", "SCORE_NEW = None", "ASSOC_THRESHOLD_LOW = None", "MAX_AGE_LOW = 0", "SCORE_AT = 6"):
        assert re.search(r"^    %s$" % re.escape(line), trk, re.M), line


# ------------------------------------------------------------------ 7. the wrappers send what they say
def test_wrappers_resolve_their_defaults():
    from test_track_assign_cpu import _fake_context
    mi355_dt, ctx, boxes, counts = _fake_context()
    ctx.associate_tracks_scored(boxes, counts, THR, 1, GAIN, 2, 0.5)
    ctx.associate_tracks_scored(boxes, counts, THR, 1, GAIN, 2, 0.5, score_new=0.6, assoc_threshold_low=0.2, max_age_low=-1, score_at=4, track_cap=9,
                                match=ANY)
    ctx.associate_stream_tracks_scored(boxes, counts, THR, [0], 1, GAIN, 2, 0.5, max_age_low=3)
    (n0, a0), (n1, a1), (n2, a2) = ctx.lib.calls
    assert (n0, n1, n2) == ("dt_associate_tracks_scored", "dt_associate_tracks_scored", "dt_associate_stream_tracks_scored")
    assert a0[3:17] == (1, 2, 4, THR, 1, 4, GAIN, 2, 0, 6, 0.5, 0.5, THR, 0)
    assert a1[3:17] == (1, 2, 4, THR, 1, 9, GAIN, 2, ANY, 4, 0.5, 0.6, 0.2, -1)
    assert a2[3:16] == (1, 2, 4, THR, 1, GAIN, 2, 0, 6, 0.5, 0.5, THR, 3)
    assert len(a0) == 24 and len(a2) == 24
