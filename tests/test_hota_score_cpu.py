"""CPU suite: HOTA scoring ("HOTA scoring") -- the restatement tests/hota_score_ref.py on a hand example, its
bounds and chunk contract, its tables against identity scoring's, the integer rule against TrackEval's float rule (scipy where it is
installed); the host helper utility.evaluate.hota; and the header / binding / DESIGN.md agreement of the three new entries.  No GPU.
"""
import math
import os
import re

import numpy as np
import pytest

import hota_score_ref as hsr
import identity_score_ref as isr
import track_score_ref as tsr

from utility import evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 1 << 20


def figures(r):
    """evaluate.hota on one clip's restatement"""
    return evaluate.hota({k: (v if k == "thresholds" else np.asarray(v)[None]) for k, v in r.items()})


def test_thresholds_are_the_measures_own():
    t = evaluate.HOTA_THRESHOLDS
    assert t.dtype == np.float32 and len(t) == 19 and (np.diff(t) > 0).all() and t[0] == np.float32(0.05) and t[-1] == np.float32(0.95)
    assert np.array_equal(t, hsr.THRESHOLDS) and evaluate.HOTA_SCALE == S


def test_hand_example():
    """two far-apart objects, T = 4, hypotheses on the ground truth, ids swapped after frame 2: every box is found (DetA 1), and each
    of the four trajectory pairs holds 2 of the 8 matches: A = 2 / (4 + 4 - 2) = 1/3"""
    h = hsr.hand_example()
    r = hsr.hota_score(*[h[k] for k in hsr.INPUTS], acap=4, bcap=4)
    assert r["sizes"].tolist() == [4, 8, 8, 2, 2, 0, 0, 8]
    assert r["gt_tab"].tolist() == [[0, 4], [1, 4], [-1, 0], [-1, 0]] and r["hyp_tab"].tolist() == [[0, 4], [1, 4], [-1, 0], [-1, 0]]
    assert r["align"][:2, :2].tolist() == [[2 * S, 2 * S], [2 * S, 2 * S]] and int(r["align"].sum()) == 8 * S
    assert r["w"][0, :2, :2].tolist() == [[1 + (2 * S * S) // (8 * S - 2 * S), 0], [0, 1 + S // 3]]
    assert r["row_to_col"].tolist() == [[0, 1]] * 4
    assert r["tp"].tolist() == [0] * 18 + [8] and r["loc"].tolist() == [0] * 18 + [8 * S]
    assert r["pairs"][18, :2, :2].tolist() == [[2, 2], [2, 2]] and int(r["pairs"].sum()) == 8
    f = figures(r)
    for e in (f["clips"][0], f["pooled"]):
        assert e["TP"].tolist() == [8] * 19 and e["FN"].tolist() == [0] * 19 and e["FP"].tolist() == [0] * 19
        assert (e["DetA"] == 1.0).all() and (e["LocA"] == 1.0).all() and np.allclose(e["AssA"], 1 / 3., rtol=0, atol=1e-15)
        assert np.allclose(e["HOTA"], math.sqrt(1 / 3.), rtol=0, atol=1e-15) and abs(e["hota"] - math.sqrt(1 / 3.)) < 1e-15
        assert e["hota0"] == e["HOTA"][0] and e["loca0"] == 1.0 and e["deta"] == 1.0
        assert (e["gt"], e["hyp"], e["gt_tracks"], e["hyp_tracks"], e["overflow"]) == (8, 8, 2, 2, 0)


def test_perfect_tracker_and_no_hypotheses():
    s, acap, bcap = isr.scene("small")
    x = [s[k] for k in ("gt_boxes", "gt_counts", "gt_ids")]
    # every id >= 0 and distinct within a frame in this scene: scored against itself every figure is 1
    r = hsr.hota_score(*(x + x), any_label=False, acap=acap, bcap=acap)
    e = figures(r)["pooled"]
    for k in evaluate.HOTA_ARRAYS[:-1]:
        assert (e[k] == 1.0).all() and e[k.lower()] == 1.0, k
    # LocA: a box's float32 IoU with itself is 1 to a few ulps (the intersection's sides are differences of rounded sums), far less than
    # 2^-20, so every q is S or S - 1 (the hand example's boxes give S exactly: test_hand_example)
    assert (e["LocA"] <= 1.0).all() and (e["LocA"] >= 1.0 - 2.0 ** -20).all()
    assert e["TP"].tolist() == [int(r["sizes"][1])] * 19 and r["sizes"][1] > 0
    none = hsr.hota_score(*(x + [s["hyp_boxes"], np.zeros_like(s["hyp_counts"]), s["hyp_ids"]]), acap=acap, bcap=bcap)
    e = figures(none)["pooled"]
    assert int(none["w"].max()) == 0 and (none["row_to_col"] == -1).all() and int(none["align"].max()) == 0
    for k in ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr"):
        assert (e[k] == 0.0).all(), k
    assert (e["LocA"] == 1.0).all() and e["TP"].tolist() == [0] * 19 and e["FN"].tolist() == [int(none["sizes"][1])] * 19 and e["hyp"] == 0


def test_bounds_of_alignment_and_weights():
    """P <= S * min(n_a, n_b) and 1 <= W <= S + 1 where q > 0, on seeded clips, repeated ids within a frame included"""
    for name in ("small", "repeated_ids", "counts_above_cap"):
        s, _, _ = isr.scene(name)
        for any_label in (False, True):
            r = hsr.scene_ref(name, any_label)
            na, nb = r["gt_tab"][:, 1].astype(np.int64), r["hyp_tab"][:, 1].astype(np.int64)
            assert (r["align"] >= 0).all() and (r["align"] <= S * np.minimum(na[:, None], nb[None, :])).all(), name
            assert int(r["align"].max()) > 0 and int(r["w"].max()) <= S + 1 and int(r["w"].min()) == 0
            assert int((r["w"] > 0).sum()) == r["sizes"][7], "a weight >= 1 exactly where q > 0"
    s, _, _ = isr.scene("repeated_ids")
    assert any(len(set(s["gt_ids"][t, :int(s["gt_counts"][t])].tolist())) < int(s["gt_counts"][t]) for t in range(12))


def test_chunked_equals_unchunked():
    for name in ("small", "repeated_ids"):
        s, acap, bcap = isr.scene(name)
        T = s["gt_boxes"].shape[0]
        whole = hsr.scene_ref(name, False)
        for chunks in ([1, 7, T - 8], [T - 1, 1]):
            got = hsr.hota_score(*[s[k] for k in hsr.INPUTS], acap=acap, bcap=bcap, chunks=chunks)
            for k in hsr.ALL_KEYS:
                assert np.array_equal(got[k], whole[k]), (name, chunks, k)
    # the second pass needs the FINISHED alignment: with the alignment of the first frames only, the weights differ
    s, acap, bcap = isr.scene("small")
    x = [s[k] for k in hsr.INPUTS]
    head = hsr.hota_align(*[v[:8] for v in x], acap=acap, bcap=bcap)
    early = hsr.hota_frames(*[v[:8] for v in x], head)
    assert not np.array_equal(early["w"], hsr.scene_ref("small", False)["w"][:8])


def test_tables_equal_identity_scoring():
    for name in sorted(tsr.SCENES):
        for any_label in (False, True):
            h, i = hsr.scene_ref(name, any_label), isr.scene_ref(name, any_label)
            assert np.array_equal(h["sizes"][:7], i["sizes"][:7]), name
            assert np.array_equal(h["gt_tab"], i["gt_tab"]) and np.array_equal(h["hyp_tab"], i["hyp_tab"]), name
            assert h["sizes"][7] >= i["sizes"][7] > 0, "every pair of IoU >= 0.5 has q > 0"
            assert int(h["tp"].sum()) > 0 and len(np.flatnonzero(h["tp"])) > 3, "vacuous scene"


def test_integer_rule_against_trackeval_float_rule():
    """30 seeded clips of well-separated objects (each ground-truth box overlaps at most one hypothesis), all 19 thresholds: TP equal;
    HOTA, DetA and AssA are ratios of equal integers; LocA loses < 2^-20 per pair to the truncation of q, and is given 2^-19"""
    pytest.importorskip("scipy.optimize")
    switched = 0
    for seed in range(30):
        s = hsr.separated_clip(seed)
        x = [s[k] for k in hsr.INPUTS]
        for t in range(s["gt_boxes"].shape[0]):
            for g in range(int(s["gt_counts"][t])):
                hits = sum(1 for i in range(int(s["hyp_counts"][t]))
                           if hsr.quantise(hsr.orc.bbox_iou(s["gt_boxes"][t, g, :4], s["hyp_boxes"][t, i, :4])) > 0)
                assert hits <= 1
        r = hsr.hota_score(*x, any_label=False, acap=16, bcap=32)
        assert r["sizes"][5] == 0 and r["sizes"][6] == 0
        switched += int(r["sizes"][4] > 5)
        e = figures(r)["pooled"]
        f = hsr.trackeval_rule(*x)
        assert np.array_equal(e["TP"], f["TP"]) and e["TP"][0] > 0, seed
        for k in ("HOTA", "DetA", "AssA"):
            assert np.abs(e[k] - f[k]).max() <= 1e-12, (seed, k)
        assert np.abs(e["LocA"] - f["LocA"]).max() <= 2.0 ** -19, seed
        assert e["TP"][0] > e["TP"][-1], "vacuous: the thresholds do not separate the pairs"
    assert switched > 20, "vacuous: no identity switches"


def hand_result():
    """two clips by hand, n_thr = 2: buckets, not suffix sums"""
    sizes = np.array([[5, 10, 9, 2, 2, 1, 0, 9], [3, 4, 0, 1, 0, 0, 0, 0]], dtype=np.int32)
    gt_tab = np.array([[[7, 6], [8, 3]], [[1, 4], [-1, 0]]], dtype=np.int32)
    hyp_tab = np.array([[[0, 5], [1, 4]], [[-1, 0], [-1, 0]]], dtype=np.int32)
    tp = np.array([[2, 5], [0, 0]], dtype=np.int32)
    loc = np.array([[2 * 300000, 5 * 900000], [0, 0]], dtype=np.int64)
    pairs = np.zeros((2, 2, 2, 2), dtype=np.int32)
    pairs[0, 0] = [[1, 1], [0, 0]]
    pairs[0, 1] = [[3, 0], [0, 2]]
    return dict(sizes=sizes, gt_tab=gt_tab, hyp_tab=hyp_tab, tp=tp, loc=loc, pairs=pairs, thresholds=np.array([0.25, 0.75], dtype=np.float32))


def test_evaluate_hota_figures_and_zero_denominators():
    res = hand_result()
    out = evaluate.hota(res)
    a, b, p = out["clips"][0], out["clips"][1], out["pooled"]
    assert np.array_equal(out["thresholds"], res["thresholds"])
    assert a["TP"].tolist() == [7, 5] and a["FN"].tolist() == [3, 5] and a["FP"].tolist() == [2, 4]
    assert a["DetA"].tolist() == [7 / 12., 5 / 14.] and a["DetRe"].tolist() == [0.7, 0.5] and a["DetPr"].tolist() == [7 / 9., 5 / 9.]
    # threshold 0: m = [[4, 1], [0, 2]]; n_a = 6, 3; n_b = 5, 4
    ass0 = (4 * 4 / (6 + 5 - 4.) + 1 * 1 / (6 + 4 - 1.) + 2 * 2 / (3 + 4 - 2.)) / 7
    ass1 = (3 * 3 / (6 + 5 - 3.) + 2 * 2 / (3 + 4 - 2.)) / 5
    assert np.allclose(a["AssA"], [ass0, ass1], rtol=0, atol=1e-15)
    assert np.allclose(a["AssRe"], [(16 / 6. + 1 / 6. + 4 / 3.) / 7, (9 / 6. + 4 / 3.) / 5], rtol=0, atol=1e-15)
    assert np.allclose(a["AssPr"], [(16 / 5. + 1 / 4. + 4 / 4.) / 7, (9 / 5. + 4 / 4.) / 5], rtol=0, atol=1e-15)
    assert np.allclose(a["HOTA"], np.sqrt(np.array([7 / 12. * ass0, 5 / 14. * ass1])), rtol=0, atol=1e-15)
    assert np.allclose(a["LocA"], [(600000 + 4500000) / (7. * S), 4500000 / (5. * S)], rtol=0, atol=1e-15)
    assert a["hota"] == a["HOTA"].mean() and a["loca"] == a["LocA"].mean() and a["hota0"] == a["HOTA"][0] and a["loca0"] == a["LocA"][0]
    assert (a["gt"], a["hyp"], a["gt_tracks"], a["hyp_tracks"], a["overflow"]) == (10, 9, 2, 2, 1)
    # TrackEval's conventions where a denominator is 0: no hypotheses, no match
    assert b["TP"].tolist() == [0, 0] and b["FN"].tolist() == [4, 4] and b["FP"].tolist() == [0, 0]
    for k in ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr"):
        assert b[k].tolist() == [0.0, 0.0], k
    assert b["LocA"].tolist() == [1.0, 1.0] and not any(math.isnan(v) for k in evaluate.HOTA_ARRAYS for v in b[k])
    # pooled: the counts of all clips before the ratios
    assert p["TP"].tolist() == [7, 5] and p["gt"] == 14 and p["hyp"] == 9 and p["gt_tracks"] == 3 and p["hyp_tracks"] == 2
    assert p["DetA"].tolist() == [7 / 16., 5 / 18.] and np.allclose(p["AssA"], a["AssA"], rtol=0, atol=1e-15)
    assert np.array_equal(p["LocA"], a["LocA"])
    # the last of a resumed run
    first = dict(res, tp=res["tp"] * 0, loc=res["loc"] * 0, pairs=res["pairs"] * 0)
    q = evaluate.hota([first, res])["pooled"]
    assert all(np.array_equal(q[k], p[k]) for k in evaluate.HOTA_ARRAYS) and q["hota"] == p["hota"]
    empty = evaluate.hota(dict(sizes=np.zeros((0, 8), dtype=np.int32), gt_tab=np.zeros((0, 2, 2), dtype=np.int32),
                               hyp_tab=np.zeros((0, 2, 2), dtype=np.int32), tp=np.zeros((0, 2), dtype=np.int32),
                               loc=np.zeros((0, 2), dtype=np.int64), pairs=np.zeros((0, 2, 2, 2), dtype=np.int32),
                               thresholds=res["thresholds"]))
    assert empty["clips"] == [] and empty["pooled"]["hota"] == 0.0 and empty["pooled"]["loca"] == 1.0
    assert "TrackEval" in evaluate.hota.__doc__ and "nan" in evaluate.hota.__doc__


LEAD = (r"dt_ctx \*ctx, const float \*d_gt_boxes, const int \*d_gt_counts, const int \*d_gt_ids, int gcap,\s*"
        r"const float \*d_hyp_boxes, const int \*d_hyp_counts, const int \*d_hyp_ids, int hcap, int id_stride, int hyp_label_at,\s*"
        r"int n_clips, int T, int flags, int acap, int bcap,\s*")
DECLS = {
    "dt_hota_align": (r"DT_API int dt_hota_align\(" + LEAD + r"int \*d_sizes, int \*d_gt_tab, int \*d_hyp_tab, int64_t \*d_align\);", 20),
    "dt_hota_weights": (r"DT_API int dt_hota_weights\(" + LEAD +
                        r"const int \*d_sizes, const int \*d_gt_tab, const int \*d_hyp_tab, const int64_t \*d_align,\s*"
                        r"int \*d_w, int \*d_dims, int \*d_gt_ent, int \*d_hyp_ent\);", 24),
    "dt_hota_count": (r"DT_API int dt_hota_count\(dt_ctx \*ctx, const float \*d_gt_boxes, int gcap, const float \*d_hyp_boxes, int hcap, int n_clips, int T,\s*"
                      r"const int \*d_dims, const int \*d_gt_ent, const int \*d_hyp_ent, const int \*d_row_to_col,\s*"
                      r"const float \*h_thresholds, int n_thr, int acap, int bcap, int flags,\s*"
                      r"int \*d_tp, int64_t \*d_loc, int \*d_pairs\);", 19),
}


def test_header_binding_and_design_agree():
    import mi355_dt
    header = open(os.path.join(ROOT, "include", "mi355_dt.h")).read()
    src = open(os.path.join(ROOT, "object_tracking_amd", "mi355_dt.py")).read()
    for name, (pattern, n_args) in DECLS.items():
        assert re.search(pattern, header), name
        assert name in mi355_dt.SYMBOLS
        args = re.search(r"L\.%s\.argtypes = \[(.*)\]" % name, src).group(1).split(", ")
        decl = re.search(r"DT_API int %s\(([^;]*)\);" % name, header).group(1)
        kinds = ["vp" if "*" in a else "cf" if a.strip().startswith("float") else "ci" for a in decl.split(",")]
        assert args == kinds and len(args) == n_args, name
    # the first two take dt_track_score's input arguments up to T, name for name
    lead = lambda name: [a.strip() for a in re.search(r"DT_API int %s\(([^;]*)\);" % name, header).group(1).split(",")][:13]
    assert lead("dt_hota_align") == lead("dt_track_score") == lead("dt_hota_weights") and lead("dt_hota_align")[-1] == "int T"
    assert re.search(r"#define DT_HOTA_MAX_THR 32\b", header) and mi355_dt.DT_HOTA_MAX_THR == 32
    for method in ("hota_align", "hota_weights", "hota_count", "hota_score"):
        assert callable(getattr(mi355_dt.Context, method)), method
    abi = re.search(r"/\* ABI version of this header.*?\*/", header, re.S).group(0)
    assert "and the three HOTA scoring entries dt_hota_align, dt_hota_weights, dt_hota_count" in abi
    assert "and the two identity scoring entries dt_identity_overlap, dt_assign_max" in abi and "the number stayed" in abi and "1.08" in abi
    assert "IDF1 / HOTA" not in header and not re.search(r"Not done here:[^.]*HOTA,", header)
    build = open(os.path.join(ROOT, "object_tracking_amd", "build.py")).read()
    assert re.search(r'"hota\.hip": \["-ffp-contract=off"\]', build)
    kernel = open(os.path.join(ROOT, "object_tracking_amd", "csrc", "hota.hip")).read()
    assert "bbox_iou_ref(" in kernel and "float bbox_iou_ref(" not in kernel and "open_trajectories(" in kernel
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "72 `dt_*` entry points up to detection scoring, 74 with identity scoring, 77 with HOTA scoring" in design
    assert "A9f" in design and "**HOTA scoring (" in design and "**Identity scoring (" in design and "IDF1 / HOTA" not in design
    for word in ("dt_hota_align", "dt_hota_weights", "dt_hota_count", "hota_align_kernel", "hota_weights_kernel", "hota_count_kernel",
                 "2 `acap` + 2 `bcap` + 9 `gcap` + 9 `hcap`", "2 `acap` + 2 `bcap` + 7 `gcap` + 7 `hcap`", "S · min(n_a, n_b)", "S + 1"):
        assert word in design, word
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "no HOTA" not in integration and "dt_hota_align" in integration and "evaluate.hota" in integration
    declared = set(re.findall(r"DT_API[^;(]*?\b(dt_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 77 and {"dt_hota_align", "dt_hota_weights", "dt_hota_count"} <= declared
    from models_tracking.MultiObjDetTracker import MultiObjDetTracker
    assert callable(MultiObjDetTracker.hota)
