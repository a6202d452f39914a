"""Track assignment: the restatement tests/track_assign_ref.py against the restatements it builds on, the
properties the optimal match must have, and the declarations.  No device.
"""
import os
import re

import numpy as np
import pytest

import identity_score_ref as isr
import track_assign_ref as tar
import track_match_ref as tmr

THR, GAIN = tar.THR, tar.GAIN
BEST, ANY = tmr.MATCH_BEST_FIRST, tmr.MATCH_ANY_LABEL


# ------------------------------------------------------------------ 1. the smallest case
def test_worked_example():
    """two boxes compete for one track: every greedy policy opens a third id, the assignment keeps both tracks"""
    boxes, counts = tar.worked_example()
    for tcap in (2, 80):
        opt = tar.associate_tracks_assign(boxes, counts, THR, 0, 0.0, 1, 0, tcap)
        assert opt["ids"].tolist() == [[0, 1], [1, 0]] and opt["nids"] == 2
        assert opt["log"][1][2] > opt["log"][1][3]      # 0.4286 + 0.4815 against 0.6667
        for match in range(4):
            old = tmr.associate_tracks_match(boxes, counts, THR, 0, 0.0, 1, match, tcap)
            assert old["ids"].tolist() == [[0, 1], [0, 2]] and old["nids"] == 3, match
    tr = tar.TrackAssign(2, THR, 0.0)
    tr.frame(boxes[0], 0)
    cand = tr.candidates(boxes[1], 0)
    assert sorted(cand) == [(0, 0), (0, 1), (1, 0)]
    assert [round(float(cand[k]), 4) for k in sorted(cand)] == [0.6667, 0.4286, 0.4815]


def test_weight_is_one_plus_the_truncated_scaled_iou():
    assert tar.weight(np.float32(1.0)) == 1 + tar.ASSIGN_IOU_SCALE and tar.weight(np.float32(0.0)) == 1
    assert tar.weight(np.float32(0.75) - np.float32(2.0 ** -24)) == 1 + 786431      # truncation, not rounding


# ------------------------------------------------------------------ 2. the solver's restatement is optimal
def test_assign_max_equals_brute_force_on_sparse_matrices():
    rs = np.random.RandomState(5)
    for k in range(300):
        r, c = rs.randint(1, 6), rs.randint(1, 6)
        w = rs.randint(1, 1 + tar.ASSIGN_IOU_SCALE, size=(r, c)) * (rs.rand(r, c) > 0.4)
        r2c, c2r, total = isr.assign_max(w)
        isr.check_assignment(w, r, c, r2c, c2r, total)
        assert total == isr.brute_force(w), (k, w.tolist())


@pytest.mark.parametrize("match", [0, ANY])
@pytest.mark.parametrize("name", sorted(tar.SCENES))
def test_optimal_pairs_weigh_at_least_best_firsts(name, match):
    """per frame, on the same table: the summed weight of the assignment's pairs is never below best-first's"""
    r = tar.scene_ref(name, match)
    assert len(r["log"]) == tar.SCENES[name][0] and r["dropped"] == 0
    assert all(opt >= bf for _, _, opt, bf, _ in r["log"])


@pytest.mark.parametrize("name", sorted(tar.SCENES))
def test_scenes_are_not_vacuous(name):
    """at the match the scene is stated at: some frame's ids differ from best-first's, some frame has more boxes than entries"""
    T, cap, _, tcap, max_age, _, match, form = tar.SCENES[name]
    assert tar.form_of(tcap, T) == form
    boxes, counts = tar.scene(name)
    r = tar.scene_ref(name, match)
    bf = tmr.associate_tracks_match(boxes, counts, THR, max_age, GAIN, 1, BEST | match, tcap)
    assert any(not np.array_equal(r["ids"][t], bf["ids"][t]) for t in range(T))
    assert any(n > nt > 0 for n, nt, _, _, _ in r["log"])
    assert any(opt > b for _, _, opt, b, _ in r["log"])


# ------------------------------------------------------------------ 3. where the match is the same, everything is
def test_sparse_scene_equals_the_decode_order_match():
    boxes, counts = tar.case_boxes("longer_than_64_frames")
    tcap = tar.CASES["longer_than_64_frames"][3]
    new = tar.ref("longer_than_64_frames", boxes, counts, 3, 2, 0, tcap)
    old = tmr.associate_tracks_match(boxes, counts, THR, 3, GAIN, 2, 0, tcap)
    for key in tar.KEYS:
        assert np.array_equal(new[key], old[key]), key


# ------------------------------------------------------------------ 4. chunks
@pytest.mark.parametrize("name", sorted(tar.SCENES))
def test_chunked_runs_equal_the_whole_clip(name):
    T, cap, _, tcap, max_age, _, match, _ = tar.SCENES[name]
    boxes, counts = tar.scene(name)
    whole = tar.scene_ref(name, match, min_hits=2)
    for chunks in ([1] * T, [T // 3, T - T // 3]):
        got = tar.associate_tracks_assign_chunked(boxes, counts, THR, max_age, GAIN, 2, match, tcap, chunks)
        for key in tar.KEYS:
            assert np.array_equal(got[key], whole[key]), (chunks, key)


def test_chunks_through_other_entries_change_the_run():
    name = "crowd_reg_grow"
    T, cap, _, tcap, max_age, _, match, _ = tar.SCENES[name]
    boxes, counts = tar.scene(name)
    q = T // 4
    chunks = [q, q, q, T - 3 * q]
    mixed = tar.associate_tracks_assign_chunked(boxes, counts, THR, max_age, GAIN, 2, match, tcap, chunks, match_at={1: BEST}, motion_at=(2,))
    assert not np.array_equal(mixed["ids"], tar.scene_ref(name, match)["ids"])
    assert (mixed["hits"][2 * q:3 * q] == -1).all() and len(mixed["log"]) == T - 2 * q


# ------------------------------------------------------------------ 5. the order of a frame's boxes
@pytest.mark.parametrize("match", [0, ANY])
@pytest.mark.parametrize("name", ["crowd_reg_grow", "crowd_reg", "crowd_lds"])
def test_shuffled_frames_give_the_same_tracks(name, match):
    T, cap, _, tcap, max_age, _, _, _ = tar.SCENES[name]
    boxes, counts = tar.scene(name)
    shuffled = tmr.permute_frames(boxes, counts, seed=11)
    a = tar.scene_ref(name, match)
    b = tar.associate_tracks_assign(shuffled, counts, THR, max_age, GAIN, 1, match, tcap)
    assert a["nids"] == b["nids"]
    assert tmr.partition(a["ids"], boxes, counts) == tmr.partition(b["ids"], shuffled, counts)


# ------------------------------------------------------------------ 6. the declarations
def test_header_and_bindings_declare_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mi355_dt.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert re.search(r"dt_associate_tracks_assign\(dt_ctx \*ctx, const float \*d_boxes, const int \*d_counts, int n_clips, int T, int cap, "
                     r"float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match, int \*d_ids, int \*d_nids, "
                     r"int \*d_gaps, int \*d_hits, float \*d_tracks, int \*d_tinfo, int \*d_tcounts\)", flat)
    assert re.search(r"dt_associate_stream_tracks_assign\(dt_ctx \*ctx, const float \*d_boxes, const int \*d_counts, int n, int T, int cap, "
                     r"float thr, int max_age, float gain, int min_hits, int match, const int \*h_slots, int \*d_ids, int \*d_nids, "
                     r"int \*d_gaps, int \*d_hits, float \*d_tracks, int \*d_tinfo, int \*d_tcounts\)", flat)
    assert int(re.search(r"#define DT_ASSIGN_IOU_SCALE (\d+)", header).group(1)) == tar.ASSIGN_IOU_SCALE == 1 << 20
    src = open(os.path.join(root, "object_tracking_amd", "mi355_dt.py")).read()
    assert '"dt_associate_tracks_assign"' in src and '"dt_associate_stream_tracks_assign"' in src
    assert int(re.search(r"^DT_ASSIGN_IOU_SCALE = (\d+)", src, re.M).group(1)) == tar.ASSIGN_IOU_SCALE
    trk = open(os.path.join(root, "object_tracking_amd", "models_tracking", "MultiObjDetTracker.py")).read()
    assert re.search(r"^    MATCH_OPTIMAL = False$", trk, re.M)


# ------------------------------------------------------------------ 7. assign=False calls what it always called
class _Lib(object):
    """stands for the library: every entry returns 0 and is noted"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _fake_context():
    import torch
    import mi355_dt

    class OnDevice(torch.Tensor):
        is_cuda = True

    ctx = object.__new__(mi355_dt.Context)
    ctx.torch, ctx.device, ctx.lib, ctx.h = torch, "cpu", _Lib(), None
    ctx._sync_stream = lambda: None
    boxes = torch.zeros((1, 2, 4, 8)).as_subclass(OnDevice)
    counts = torch.zeros((1, 2), dtype=torch.int32)
    return mi355_dt, ctx, boxes, counts


def test_assign_false_sends_nothing_new():
    mi355_dt, ctx, boxes, counts = _fake_context()
    names = lambda: [c[0] for c in ctx.lib.calls]
    ctx.associate_tracks(boxes, counts, THR, 1, GAIN, 1)
    ctx.associate_tracks(boxes, counts, THR, 1, GAIN, 1, match=ANY)
    ctx.associate_tracks(boxes, counts, THR, 1, GAIN, 1, match=4)
    ctx.associate_stream_tracks(boxes, counts, THR, [0], 1, GAIN, 1)
    ctx.associate_stream_tracks(boxes, counts, THR, [0], 1, GAIN, 1, match=BEST)
    assert names() == ["dt_associate_tracks", "dt_associate_tracks_match", "dt_associate_tracks_match", "dt_associate_stream_tracks",
                       "dt_associate_stream_tracks_match"]
    assert ctx.lib.calls[2][1][11] == 4      # match = 4 still reaches the match entry, which refuses it
    del ctx.lib.calls[:]
    ctx.associate_tracks(boxes, counts, THR, 1, GAIN, 1, assign=True)
    ctx.associate_tracks(boxes, counts, THR, 1, GAIN, 1, match=BEST | ANY, assign=True)
    ctx.associate_stream_tracks(boxes, counts, THR, [0], 1, GAIN, 1, match=ANY, assign=True)
    assert names() == ["dt_associate_tracks_assign", "dt_associate_tracks_assign", "dt_associate_stream_tracks_assign"]
    assert [c[1][11 if c[0].endswith("tracks_assign") and "stream" not in c[0] else 10] for c in ctx.lib.calls] == [0, BEST | ANY, ANY]
