"""CPU suite: detection scoring ("Detection scoring") -- the restatement tests/detect_score_ref.py against the
numbers of the worked example and its own invariants, the host helpers of utility/evaluate.py against the restatement's loop-form
AP, and the header / binding / document agreement of the two new entries.  No GPU.
"""
import math
import os
import re

import numpy as np
import pytest

import detect_score_ref as dsr

from utility import evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_SCENES = ("registers", "passes", "thr16", "nc80", "edges", "odd_grid")      # (rank_tiles is the GPU suite's: its restatement takes seconds)


def test_worked_example():
    """DESIGN.md's two frames, exactly"""
    s = dsr.worked_example()
    r = dsr.detect_score(s, 1, (0.5,))
    assert r["state"][0].tolist() == dsr.WORKED_STATE
    assert r["rank"][0].tolist() == dsr.WORKED_RANK and r["ctp"][0].tolist() == dsr.WORKED_CTP
    assert r["best"].tolist() == [[0, 0, 1, 0], [0, -1, -1, -1]]           # the box that overlaps nothing still has candidates: row 0 at IoU 0
    assert r["iou"][0, 1] == np.float32(7) / np.float32(9) and r["iou"][0, 3] == 0 and r["iou"][0, 0] == 1 and r["iou"][0, 2] == 1
    assert (int(r["ngt"][0]), int(r["ndet"][0, 0]), int(r["ntp"][0, 0])) == (dsr.WORKED_NGT, dsr.WORKED_NDET, dsr.WORKED_NTP)
    assert dsr.curve(r, 0, 0) == [0, 1, 2, 2]
    for method in dsr.METHODS:
        a = evaluate.average_precision(r, method)
        assert abs(a["ap"][0, 0] - dsr.WORKED_AP) < 1e-12 and abs(a["map"][0] - dsr.WORKED_AP) < 1e-12 and abs(a["map_all"] - dsr.WORKED_AP) < 1e-12
        assert abs(dsr.average_precision(r, method)[0][0][0] - dsr.WORKED_AP) < 1e-12
    pr = evaluate.precision_recall(r, 0, 0)
    assert np.allclose(pr["precision"], [0, 1 / 2., 2 / 3., 1 / 2.], rtol=1e-15) and pr["recall"].tolist() == [0, 0.5, 1, 1]
    assert pr["scores"].tolist() == [np.float32(v) for v in (0.95, 0.9, 0.85, 0.8)] and pr["tp"].tolist() == [0, 1, 2, 2]


def test_detections_equal_to_ground_truth_give_ap_1():
    """... for every class present, at every COCO threshold (not at 1.0: in float32 a box's IoU with itself may be 1 - 4e-7); the scene's exact duplicates are taken out first: twins share their
    best row, the lowest, so one of them would be a duplicate FP"""
    s = dsr.make_scene(6, 24, 24, 5, 12, 21)
    keep = []
    for b in range(6):                               # one row of every set of exact duplicates
        seen, rows = set(), []
        for g in range(int(s["gt_counts"][b])):
            key = s["gt_boxes"][b, g, :6].tobytes()
            if key not in seen:
                seen.add(key)
                rows.append(s["gt_boxes"][b, g].copy())
        keep.append(rows)
    det = np.zeros((6, 24, 8), dtype=np.float32)
    cnt = np.array([len(r) for r in keep], dtype=np.int32)
    for b, rows in enumerate(keep):
        det[b, :len(rows)] = rows
    own = dict(det_boxes=det, det_counts=cnt, gt_boxes=det.copy(), gt_counts=cnt, gt_flags=None)
    r = dsr.detect_score(own, 5, dsr.COCO, flags=False)
    a = evaluate.average_precision(r, "area")
    present = r["ngt"] > 0
    assert present.sum() >= 3 and (a["ap"][:, present] == 1.0).all() and (a["map"] == 1.0).all() and a["map_all"] == 1.0
    for method in ("voc11", "coco101"):
        assert np.allclose(evaluate.average_precision(r, method)["ap"][:, present], 1.0, rtol=1e-15)


@pytest.mark.parametrize("name", CPU_SCENES)
def test_average_precision_against_the_loop_form(name):
    r = dsr.scene_ref(name)
    for method in dsr.METHODS:
        got = evaluate.average_precision(r, method)
        ap, maps, map_all = dsr.average_precision(r, method)
        np.testing.assert_allclose(got["ap"], np.array(ap), rtol=1e-12, atol=0, equal_nan=True)
        np.testing.assert_allclose(got["map"], np.array(maps), rtol=1e-12, atol=0, equal_nan=True)
        np.testing.assert_allclose(got["map_all"], map_all, rtol=1e-12, atol=0, equal_nan=True)
        assert np.array_equal(np.isnan(got["ap"]), np.tile(r["ngt"] == 0, (got["ap"].shape[0], 1)))
    assert 0 < got["map"][0] < 1, "a scene with misses and false positives"
    k, c = 0, int(np.argmax(r["ndet"][0]))
    pr = evaluate.precision_recall(r, k, c)
    assert pr["tp"].tolist() == dsr.curve(r, k, c) and (np.diff(pr["scores"]) <= 0).all()


def test_nan_and_zero_handling():
    s = dsr.worked_example()
    # three classes: 0 as in the example; 1 has ground truth and no detection -> 0; 2 has a detection and no ground truth -> nan
    s["gt_boxes"][1, 0, 5] = 1
    s["det_boxes"][1, 0, 5] = 2
    r = dsr.detect_score(s, 3, (0.5, 0.9))
    assert r["ngt"].tolist() == [1, 1, 0] and r["ndet"][0].tolist() == [3, 0, 1] and r["state"][0, 1, 0] == 0 and r["best"][1, 0] == -1
    for method in dsr.METHODS:
        a = evaluate.average_precision(r, method)
        assert a["ap"][0, 1] == 0.0 and math.isnan(a["ap"][0, 2]) and a["ap"][0, 0] > 0
        assert abs(a["map"][0] - a["ap"][0, 0] / 2) < 1e-15, "the class without ground truth is left out of the mean, the one without detections is not"
        ap, maps, _ = dsr.average_precision(r, method)
        assert ap[0][1] == 0.0 and math.isnan(ap[0][2])
    empty = dsr.all_empty()
    r = dsr.detect_score(empty, 2, (0.5,))
    a = evaluate.average_precision(r)
    assert np.isnan(a["ap"]).all() and np.isnan(a["map"]).all() and math.isnan(a["map_all"])
    assert (r["state"] == -1).all() and (r["rank"] == -1).all() and r["ngt"].tolist() == [0, 0]


def test_a_nan_iou_is_below_no_threshold():
    r = dsr.detect_score(dsr.zero_area(), 1, (0.5, 1.0))
    assert np.isnan(r["iou"][0, :2]).all() and r["iou"][0, 2] == 0 and r["best"][0].tolist() == [0, 0, 0, -1]
    assert r["state"][:, 0].tolist() == [[0, 1, 0, -1]] * 2 and r["rank"][0, 0].tolist() == [1, 0, 2, -1] and r["ctp"][0, 0].tolist() == [1, 1, 1, -1]


def test_restatement_chunk_contract():
    s, NC, thr = dsr.scene("passes")
    whole = dsr.scene_ref("passes")
    B = s["det_boxes"].shape[0]
    m = dsr.detect_match(s["det_boxes"], s["det_counts"], s["gt_boxes"], s["gt_counts"], s["gt_flags"], NC, thr, chunks=[1, 3, B - 4])
    for k in ("state", "best", "iou"):
        assert np.array_equal(m[k], whole[k]), k
    rk = dsr.detect_rank(s["det_boxes"], s["det_counts"], m["state"], s["gt_boxes"], s["gt_counts"], s["gt_flags"], NC)
    for k in ("rank", "ctp", "ngt", "ndet", "ntp"):
        assert np.array_equal(rk[k], whole[k]), k
    # ... while the rank of a chunk alone is another ranking
    part = dsr.detect_rank(s["det_boxes"][:4], s["det_counts"][:4], m["state"][:, :4], s["gt_boxes"][:4], s["gt_counts"][:4], s["gt_flags"][:4], NC)
    assert not np.array_equal(part["rank"], whole["rank"][:, :4])


def test_the_parallel_form_of_the_walk():
    """what the match kernel relies on: detection i is a duplicate at threshold k exactly when a detection before it in the frame's
    score order has the same best row and an IoU >= thr[k]"""
    for name in ("registers", "passes", "edges"):
        s, NC, _ = dsr.scene(name)
        r = dsr.scene_ref(name, dsr.COCO)
        B, cap, _ = s["det_boxes"].shape
        for b in range(B):
            nd = min(max(int(s["det_counts"][b]), 0), cap)
            for i in range(nd):
                if r["state"][0, b, i] < 0:
                    continue
                prior = -1.0
                for j in range(nd):
                    sj, si = s["det_boxes"][b, j, 6], s["det_boxes"][b, i, 6]
                    if r["best"][b, j] >= 0 and r["best"][b, j] == r["best"][b, i] and (sj > si or (sj == si and j < i)):
                        prior = max(prior, r["iou"][b, j])
                for k, thr in enumerate(dsr.COCO):
                    thr = np.float32(thr)
                    if r["best"][b, i] < 0 or r["iou"][b, i] < thr:
                        want = 0
                    elif s["gt_flags"][b, r["best"][b, i]] & 1:
                        want = 2
                    else:
                        want = 0 if prior >= thr else 1
                    assert r["state"][k, b, i] == want, (name, b, i, k)


@pytest.mark.parametrize("name", CPU_SCENES)
def test_scenes_are_not_vacuous(name):
    c = dsr.coverage(name)
    for what, n in c.items():
        assert n > 0, (name, what, c)


def test_edge_scenes_hold_their_edges():
    s, _, _ = dsr.scene("edges")
    cap, gcap = s["det_boxes"].shape[1], s["gt_boxes"].shape[1]
    assert (s["det_counts"] > cap).any() and (s["gt_counts"] > gcap).any()
    assert s["det_counts"][1] == 0 and s["gt_counts"][1] > 0 and s["det_counts"][2] > 0 and s["gt_counts"][2] == 0
    assert s["det_counts"][3] == 0 and s["gt_counts"][3] == 0
    assert (s["gt_flags"] == 2).any() and (s["gt_flags"] == 3).any(), "bit 0 alone decides"
    s, _, _ = dsr.scene("passes")
    assert s["det_counts"].max() > 64 and s["gt_counts"].max() > 64
    s, NC, _ = dsr.scene("nc80")
    assert NC == 80 and (dsr.scene_ref("nc80")["ngt"] == 0).sum() >= 70


def test_ranking_by_conf_is_another_ranking():
    a, b = dsr.scene_ref("registers"), dsr.scene_ref("registers", score_at=4)
    assert np.array_equal(a["best"], b["best"]) and not np.array_equal(a["rank"], b["rank"])


def test_gt_from_annotations():
    labels = ["person", "car", "dog"]
    records = [dict(width=640, height=480, filename="a.jpg",
                    object=[dict(name="car", xmin=100, ymin=50, xmax=140, ymax=130),
                            dict(name="cat", xmin=0, ymin=0, xmax=10, ymax=10),                  # not a label: dropped
                            dict(name="dog", xmin=600, ymin=400, xmax=640, ymax=480, difficult=1)]),
               dict(width=320, height=240, filename="b.jpg", object=[dict(name="person", xmin=0, ymin=0, xmax=320, ymax=240, difficult=0)])]
    boxes, counts, flags = evaluate.gt_from_annotations(records, labels, gcap=3)
    assert boxes.shape == (2, 3, 8) and boxes.dtype == np.float32 and counts.dtype == np.int32 and flags.dtype == np.int32
    assert counts.tolist() == [2, 1] and flags.tolist() == [[0, 1, 0], [0, 0, 0]]
    assert np.allclose(boxes[0, 0, :7], [120 / 640., 90 / 480., 40 / 640., 80 / 480., 1, 1, 1])
    assert np.allclose(boxes[0, 1, :7], [620 / 640., 440 / 480., 40 / 640., 80 / 480., 1, 2, 1])
    assert boxes[1, 0, :6].tolist() == [0.5, 0.5, 1, 1, 1, 0] and (boxes[0, 2] == 0).all()
    with pytest.raises(ValueError):
        evaluate.gt_from_annotations(records, labels, gcap=1)
    assert len(evaluate.COCO_THRESHOLDS) == 10 and evaluate.COCO_THRESHOLDS[0] == 0.5 and abs(evaluate.COCO_THRESHOLDS[-1] - 0.95) < 1e-12
    assert [float(np.float32(t)) for t in evaluate.COCO_THRESHOLDS] == [float(np.float32(t)) for t in dsr.COCO]


def test_header_binding_and_design_agree():
    import mi355_dt
    header = open(os.path.join(ROOT, "include", "mi355_dt.h")).read()
    src = open(os.path.join(ROOT, "object_tracking_amd", "mi355_dt.py")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"DT_API int dt_detect_match\(dt_ctx \*ctx, const float \*d_det_boxes, const int \*d_det_counts, int cap, int score_at,\s*"
                     r"const float \*d_gt_boxes, const int \*d_gt_counts, const int \*d_gt_flags, int gcap,\s*"
                     r"int B, int NC, const float \*h_thresholds, int n_thr,\s*"
                     r"int \*d_state, int \*d_best, float \*d_iou\);", header)
    assert re.search(r"DT_API int dt_detect_rank\(dt_ctx \*ctx, const float \*d_det_boxes, const int \*d_det_counts, int cap, int score_at, const int \*d_state,\s*"
                     r"const float \*d_gt_boxes, const int \*d_gt_counts, const int \*d_gt_flags, int gcap,\s*"
                     r"int B, int NC, int n_thr,\s*"
                     r"int \*d_rank, int \*d_ctp, int \*d_ngt, int \*d_ndet, int \*d_ntp\);", header)
    for name, count in (("dt_detect_match", 16), ("dt_detect_rank", 18)):
        assert name in mi355_dt.SYMBOLS
        args = re.search(r"L\.%s\.argtypes = \[(.*)\]" % name, src).group(1).split(", ")
        decl = re.search(r"DT_API int %s\(([^;]*)\);" % name, header).group(1)
        kinds = ["vp" if "*" in a else "cf" if a.strip().startswith("float") else "ci" for a in decl.split(",")]
        assert args == kinds and len(args) == count, name
        assert "`%s`" % name in design, name
        assert re.search(r"`%s`[^\n]*\b%d arguments" % (name, count), design), "DESIGN.md states the argument count of " + name
    comment = re.search(r"/\* ABI version of this header.*?\*/", header, re.S).group(0)
    assert "dt_detect_match, dt_detect_rank" in comment and "the number stayed" in comment
    assert re.search(r"#define DT_BOX_FLOATS 8\b", header)
    assert "72 `dt_*` entry points" in design and "A7b" in design and "Detection scoring" in design
    build = open(os.path.join(ROOT, "object_tracking_amd", "build.py")).read()
    assert re.search(r'"detscore\.hip": \["-ffp-contract=off"\]', build)
    kernel = open(os.path.join(ROOT, "object_tracking_amd", "csrc", "detscore.hip")).read()
    assert "bbox_iou_ref(" in kernel and "float bbox_iou_ref(" not in kernel, "the IoU has one definition (dt_internal.h)"
    for k in ("detect_match_kernel", "detect_rank_kernel"):
        assert k in kernel
