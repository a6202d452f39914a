"""GPU suite (-m gpu): detection scoring -- the VOC match per frame and the class-wise score order over a set, on the device
("Detection scoring").

Every integer output is compared exactly with the plain restatement tests/detect_score_ref.py, and `iou` through an int32 view:
detscore.hip forms no fused multiply-add and nothing on the device is summed in floats, so there is no tolerance anywhere.
"""
import ctypes

import numpy as np
import pytest
import torch

import detect_score_ref as dsr

from test_gpu_track_memory import dev, small_tracker

from utility import evaluate, synth

pytestmark = pytest.mark.gpu

ARG = 1
MATCH_KEYS, RANK_KEYS = ("state", "best", "iou"), ("rank", "ctp", "ngt", "ndet", "ntp")
FILL = -7


def ctx_():
    return small_tracker()[0].model.ctx


def on_dev(ctx, s, sl=slice(None), flags=True):
    """a scene dict -> (det_boxes, det_counts, gt_boxes, gt_counts, gt_flags or None) on the device, frames sl"""
    d = [dev(s[k][sl], ctx) for k in ("det_boxes", "det_counts", "gt_boxes", "gt_counts")]
    return d + [dev(s["gt_flags"][sl], ctx) if flags and s.get("gt_flags") is not None else None]


def to_host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def same(got, ref, what, keys=MATCH_KEYS + RANK_KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(ref[k])
        if k == "iou":
            g, w = g.view(np.int32), w.view(np.int32)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert np.array_equal(g, w), (what, k, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def gpu_score(ctx, s, NC, thr, flags=True, score_at=6):
    d = on_dev(ctx, s, flags=flags)
    return to_host(ctx.detect_score(d[0], d[1], d[2], d[3], NC, thresholds=thr, gt_flags=d[4], score_at=score_at))


def raw_match(ctx, d, nb_class, thresholds, fill=FILL, **over):
    """the C entry on device tensors d, every output pre-filled; `over` replaces arguments by name -> (return code, outputs)"""
    import mi355_dt
    B, cap, _ = d[0].shape
    gcap = d[2].shape[1]
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32))
    n = len(thr)
    o = dict(state=torch.full((max(n, 1), B, cap), fill, dtype=torch.int32, device=ctx.device),
             best=torch.full((B, cap), fill, dtype=torch.int32, device=ctx.device), iou=torch.full((B, cap), float(fill), device=ctx.device))
    a = dict(det_boxes=d[0], det_counts=d[1], cap=cap, score_at=6, gt_boxes=d[2], gt_counts=d[3], gt_flags=d[4], gcap=gcap, B=B, NC=nb_class,
             thr=thr.ctypes.data_as(ctypes.c_void_p), n_thr=n, state=o["state"], best=o["best"], iou=o["iou"])
    a.update(over)
    p = lambda x: mi355_dt._dptr(x) if x is None or torch.is_tensor(x) else x
    ctx._sync_stream()
    rc = ctx.lib.dt_detect_match(ctx.h, p(a["det_boxes"]), p(a["det_counts"]), a["cap"], a["score_at"], p(a["gt_boxes"]), p(a["gt_counts"]),
                                 p(a["gt_flags"]), a["gcap"], a["B"], a["NC"], a["thr"], a["n_thr"], p(a["state"]), p(a["best"]), p(a["iou"]))
    torch.cuda.synchronize()
    return rc, o


def raw_rank(ctx, d, states, nb_class, fill=FILL, **over):
    import mi355_dt
    B, cap, _ = d[0].shape
    gcap = d[2].shape[1]
    n = states.shape[0]
    i32 = lambda *s: torch.full(s, fill, dtype=torch.int32, device=ctx.device)
    o = dict(rank=i32(n, B, cap), ctp=i32(n, B, cap), ngt=i32(nb_class), ndet=i32(n, nb_class), ntp=i32(n, nb_class))
    a = dict(det_boxes=d[0], det_counts=d[1], cap=cap, score_at=6, state=states, gt_boxes=d[2], gt_counts=d[3], gt_flags=d[4], gcap=gcap, B=B,
             NC=nb_class, n_thr=n)
    a.update(o)
    a.update(over)
    p = lambda x: mi355_dt._dptr(x) if x is None or torch.is_tensor(x) else x
    ctx._sync_stream()
    rc = ctx.lib.dt_detect_rank(ctx.h, p(a["det_boxes"]), p(a["det_counts"]), a["cap"], a["score_at"], p(a["state"]), p(a["gt_boxes"]),
                                p(a["gt_counts"]), p(a["gt_flags"]), a["gcap"], a["B"], a["NC"], a["n_thr"], p(a["rank"]), p(a["ctp"]),
                                p(a["ngt"]), p(a["ndet"]), p(a["ntp"]))
    torch.cuda.synchronize()
    return rc, o


def untouched(o, fill=FILL):
    fbits = int(np.float32(fill).view(np.int32))
    return all(bool((v.view(torch.int32) == (fbits if v.dtype == torch.float32 else fill)).all()) for v in o.values())


# ------------------------------------------------------------------ 1. parity with the restatement
@pytest.mark.parametrize("name", sorted(dsr.SCENES))
def test_parity_with_restatement(name):
    s, NC, thr = dsr.scene(name)
    ref = dsr.scene_ref(name)
    B, cap, _ = s["det_boxes"].shape
    if name == "registers":
        assert (B, cap, s["gt_boxes"].shape[1], NC, len(thr)) == (5, 16, 8, 3, 1)
    if name == "passes":
        assert cap == 96 and s["gt_boxes"].shape[1] == 80 and B == 7 and NC == 12 and len(thr) == 10
        assert s["det_counts"].max() > 64 and s["gt_counts"].max() > 64
    if name == "thr16":
        assert len(thr) == 16 and NC == 1
    if name == "nc80":
        assert NC == 80 and (ref["ngt"] == 0).sum() >= 70
    if name == "edges":
        assert (s["det_counts"] > cap).any() and (s["gt_counts"] > s["gt_boxes"].shape[1]).any()
        assert s["det_counts"][1] == 0 and s["gt_counts"][2] == 0 and s["det_counts"][3] == 0 and s["gt_counts"][3] == 0
    if name == "rank_tiles":
        live = int((ref["state"][0] >= 0).sum())
        assert (B, cap) == (64, 96) and live > 5000 and abs(live / 64.0 - 80) < 12
        assert ref["ndet"][0].max() > 0.9 * ref["ndet"][0].sum(), "one class holds over 90 % of the ranked rows"
    if name == "odd_grid":
        assert (B * cap) % 256 != 0 and (B * cap) % 64 != 0
    same(gpu_score(ctx_(), s, NC, thr), ref, name)


def test_scenes_are_not_vacuous():
    for name in sorted(dsr.SCENES):
        c = dsr.coverage(name)
        assert min(c.values()) > 0, (name, c)


def test_worked_example():
    got = gpu_score(ctx_(), dsr.worked_example(), 1, (0.5,))
    assert got["state"][0].tolist() == dsr.WORKED_STATE
    assert got["rank"][0].tolist() == dsr.WORKED_RANK and got["ctp"][0].tolist() == dsr.WORKED_CTP
    assert (int(got["ngt"][0]), int(got["ndet"][0, 0]), int(got["ntp"][0, 0])) == (dsr.WORKED_NGT, dsr.WORKED_NDET, dsr.WORKED_NTP)
    for method in dsr.METHODS:
        assert abs(evaluate.average_precision(got, method)["ap"][0, 0] - dsr.WORKED_AP) < 1e-12


def test_a_nan_iou_is_below_no_threshold():
    s = dsr.zero_area()
    got = gpu_score(ctx_(), s, 1, (0.5, 1.0))
    assert got["state"][:, 0].tolist() == [[0, 1, 0, -1]] * 2 and np.isnan(got["iou"][0, :2]).all()
    same(got, dsr.detect_score(s, 1, (0.5, 1.0)), "zero-area boxes")


def test_ranking_by_conf():
    s, NC, thr = dsr.scene("registers")
    same(gpu_score(ctx_(), s, NC, thr, score_at=4), dsr.scene_ref("registers", score_at=4), "score_at 4")


def test_all_empty_set_and_no_frames():
    ctx = ctx_()
    s = dsr.all_empty()
    got = gpu_score(ctx, s, 2, (0.5, 0.75))
    same(got, dsr.detect_score(s, 2, (0.5, 0.75)), "all empty")
    assert (got["state"] == -1).all() and (got["rank"] == -1).all() and got["ngt"].tolist() == [0, 0] and not got["ndet"].any()
    # B = 0: nothing to match, and the rank still writes the totals
    d = on_dev(ctx, s, slice(0, 0))
    rc, o = raw_match(ctx, d, 2, (0.5,))
    assert rc == 0
    rc, o = raw_rank(ctx, d, torch.empty((1, 0, 8), dtype=torch.int32, device=ctx.device), 2)
    assert rc == 0 and not o["ngt"].any() and not o["ndet"].any() and not o["ntp"].any()


# ------------------------------------------------------------------ 2. flags, chunks, garbage, determinism
def test_null_flags_equal_zero_flags():
    ctx = ctx_()
    s, NC, thr = dsr.scene("passes")
    none = gpu_score(ctx, s, NC, thr, flags=False)
    zero = gpu_score(ctx, dict(s, gt_flags=np.zeros_like(s["gt_flags"])), NC, thr)
    same(none, zero, "NULL flags against zeros")
    same(none, dsr.scene_ref("passes", flags=False), "NULL flags")
    assert not np.array_equal(none["state"], dsr.scene_ref("passes")["state"]), "the scene's flags matter"


def test_chunk_contract():
    ctx = ctx_()
    s, NC, thr = dsr.scene("passes")
    ref = dsr.scene_ref("passes")
    B = s["det_boxes"].shape[0]
    parts, b0 = [], 0
    for L in (1, 7 - 2, 1):
        d = on_dev(ctx, s, slice(b0, b0 + L))
        parts.append(ctx.detect_match(d[0], d[1], d[2], d[3], NC, thresholds=thr, gt_flags=d[4]))
        b0 += L
    assert b0 == B
    m = dict(state=torch.cat([p["state"] for p in parts], dim=1).contiguous(), best=torch.cat([p["best"] for p in parts]),
             iou=torch.cat([p["iou"] for p in parts]))
    same(to_host(m), ref, "match in chunks of 1 / 5 / 1 frames", MATCH_KEYS)
    d = on_dev(ctx, s)
    same(to_host(ctx.detect_rank(d[0], d[1], m["state"], d[2], d[3], NC, gt_flags=d[4])), ref, "rank of the concatenation", RANK_KEYS)


def test_chunks_of_1_7_rest():
    """the issue's split: 1 frame, 7 frames, the rest -- on the 64-frame set"""
    ctx = ctx_()
    s, NC, thr = dsr.scene("rank_tiles")
    ref = dsr.scene_ref("rank_tiles")
    B = s["det_boxes"].shape[0]
    parts, b0 = [], 0
    for L in (1, 7, B - 8):
        d = on_dev(ctx, s, slice(b0, b0 + L))
        parts.append(ctx.detect_match(d[0], d[1], d[2], d[3], NC, thresholds=thr, gt_flags=d[4]))
        b0 += L
    m = dict(state=torch.cat([p["state"] for p in parts], dim=1).contiguous(), best=torch.cat([p["best"] for p in parts]),
             iou=torch.cat([p["iou"] for p in parts]))
    same(to_host(m), ref, "match in chunks of 1 / 7 / rest", MATCH_KEYS)
    d = on_dev(ctx, s)
    same(to_host(ctx.detect_rank(d[0], d[1], m["state"], d[2], d[3], NC, gt_flags=d[4])), ref, "rank of the concatenation", RANK_KEYS)


def test_every_word_is_overwritten_and_twice_gives_the_same_bits():
    ctx = ctx_()
    for name in ("edges", "odd_grid"):
        s, NC, thr = dsr.scene(name)
        ref = dsr.scene_ref(name)
        d = on_dev(ctx, s)
        runs = []
        for fill in (FILL, 0x5a5a5a5a):
            rc, m = raw_match(ctx, d, NC, thr, fill=fill)
            assert rc == 0
            rc, r = raw_rank(ctx, d, m["state"], NC, fill=fill)
            assert rc == 0
            m.update(r)
            runs.append(to_host(m))
            same(runs[-1], ref, "%s, outputs pre-filled with %d" % (name, fill))
        same(runs[0], runs[1], name + " twice")


def test_rank_reads_two_bits_of_a_state():
    """state words other than -1, 0, 1, 2 cannot come from the match; the rank keeps to their low two bits and to the rows in use"""
    ctx = ctx_()
    s, NC, thr = dsr.scene("registers")
    d = on_dev(ctx, s)
    st = dev(dsr.scene_ref("registers")["state"], ctx).clone()
    B, cap, _ = s["det_boxes"].shape
    for b in range(B):
        st[:, b, min(max(int(s["det_counts"][b]), 0), cap):] = 1          # rows beyond the count: not read
    rc, o = raw_rank(ctx, d, st, NC)
    assert rc == 0
    same(to_host(o), dsr.scene_ref("registers"), "states beyond the count", RANK_KEYS)


# ------------------------------------------------------------------ 3. argument errors
def test_argument_errors_leave_the_outputs_untouched():
    ctx = ctx_()
    s, NC, thr = dsr.scene("registers")
    d = on_dev(ctx, s)
    B, cap, _ = s["det_boxes"].shape
    nan = float("nan")
    keep = [np.asarray(v, dtype=np.float32) for v in ((0.0,), (1.5,), (nan,), (0.5, -0.1))]
    bad_match = [dict(det_boxes=None), dict(det_counts=None), dict(gt_boxes=None), dict(gt_counts=None), dict(thr=None), dict(state=None),
                 dict(best=None), dict(iou=None), dict(B=-1), dict(cap=0), dict(gcap=0), dict(gcap=-3), dict(NC=0), dict(n_thr=0), dict(n_thr=17),
                 dict(score_at=-1), dict(score_at=8), dict(B=1 << 20, cap=1 << 11), dict(B=1 << 20, gcap=1 << 11),
                 dict(cap=13654, gcap=1), dict(cap=1, gcap=6827)]      # 3 * cap + 6 * gcap = 40968 > 40960 words
    bad_match += [dict(thr=k.ctypes.data_as(ctypes.c_void_p), n_thr=len(k)) for k in keep]
    for over in bad_match:
        rc, o = raw_match(ctx, d, NC, thr, **over)
        assert rc == ARG and untouched(o), over
    assert "LDS" in ctx.lib.dt_last_error(ctx.h).decode() or "threshold" in ctx.lib.dt_last_error(ctx.h).decode()
    state = dev(dsr.scene_ref("registers")["state"], ctx)
    bad_rank = [dict(det_boxes=None), dict(det_counts=None), dict(state=None), dict(gt_boxes=None), dict(gt_counts=None), dict(rank=None),
                dict(ctp=None), dict(ngt=None), dict(ndet=None), dict(ntp=None), dict(B=-1), dict(cap=0), dict(gcap=0), dict(NC=0), dict(NC=-2),
                dict(n_thr=0), dict(n_thr=17), dict(score_at=8), dict(B=1 << 20, cap=1 << 11), dict(B=1 << 20, gcap=1 << 11)]
    for over in bad_rank:
        rc, o = raw_rank(ctx, d, state, NC, **over)
        assert rc == ARG and untouched(o), over
    # ... and the same call without a bad argument runs
    rc, o = raw_match(ctx, d, NC, thr)
    assert rc == 0 and not untouched(o)
    assert ctx.lib.dt_abi_version() == 108


def test_cap_1024_at_16_thresholds():
    """the largest frame the issue names: cap = gcap = 1024, n_thr = 16 -- one crowded frame and one empty one"""
    ctx = ctx_()
    key = "cap1024"
    if key not in dsr._SCENES:
        s = dsr.make_scene(2, 1024, 1024, 3, 150, 31)
        dsr._SCENES[key] = (s, 3, tuple(0.2 + 0.05 * i for i in range(16)))
    s, NC, thr = dsr.scene(key)
    assert s["det_boxes"].shape[1] == 1024 and s["gt_boxes"].shape[1] == 1024 and s["det_counts"].max() > 128
    same(gpu_score(ctx, s, NC, thr), dsr.scene_ref(key), "cap 1024")


# ------------------------------------------------------------------ 4. end to end
def end_to_end_inputs():
    """KerasYOLO.detect on four synthetic frames at 416 x 416 and ground truth made of a subset of its own boxes plus jittered copies
    -> (detector, detect() result, its boxes and counts on the host, gt_boxes, gt_counts, gt_flags)"""
    from models_detection.KerasYOLO import KerasYOLO
    C = 12
    det = KerasYOLO({'LABELS': [str(i) for i in range(C)], 'BATCH_SIZE': 4, 'IMAGE_H': 416, 'IMAGE_W': 416, 'GRID_H': 13, 'GRID_W': 13},
                    weights=synth.synth_darknet_blob(C))
    frames = synth.synth_clip(4, 416, 416, 3, seed=23)
    for thr in (0.3, 0.1, 0.05, 0.02, 0.01):           # a threshold low enough that every frame has boxes
        det.OBJ_THRESHOLD = thr
        res = det.detect(frames)
        if int(res["counts"].min()) >= 8:
            break
    boxes, counts = res["boxes"].cpu().numpy(), res["counts"].cpu().numpy()
    cap = boxes.shape[1]
    print("end to end: OBJ_THRESHOLD %g, boxes per frame %s" % (thr, counts.tolist()))
    assert counts.min() >= 8, "vacuous without boxes: %s" % counts.tolist()
    assert np.isfinite(boxes).all() and np.isfinite(boxes[:, :, 2] * boxes[:, :, 3]).all(), "the rule wants finite boxes and areas"
    rs = np.random.RandomState(9)
    gcap = 64
    gt_boxes = np.zeros((4, gcap, 8), dtype=np.float32)
    gt_counts = np.zeros(4, dtype=np.int32)
    gt_flags = np.zeros((4, gcap), dtype=np.int32)
    for b in range(4):
        n = min(int(counts[b]), cap)
        rows = []
        for i in rs.permutation(n)[:min(n, 40)]:
            if rs.rand() < 0.6:                          # a subset of its own boxes ...
                rows.append(boxes[b, i].copy())
            if rs.rand() < 0.5:                          # ... and jittered copies
                r = boxes[b, i].copy()
                r[:2] += ((rs.rand(2) - .5) * .04).astype(np.float32)
                r[2:4] *= (1 + (rs.rand(2) - .5) * .3).astype(np.float32)
                rows.append(r)
        rows = rows[:gcap]
        for g, r in enumerate(rows):
            gt_boxes[b, g] = r
            gt_flags[b, g] = int(rs.rand() < 0.1)
        gt_counts[b] = len(rows)
    return det, res, boxes, counts, gt_boxes, gt_counts, gt_flags


def test_keras_yolo_score_end_to_end():
    """KerasYOLO.score -> average_precision equals the restatement fed the same device boxes"""
    C = 12
    det, res, boxes, counts, gt_boxes, gt_counts, gt_flags = end_to_end_inputs()
    thr = evaluate.COCO_THRESHOLDS
    got = det.score(res, (gt_boxes, gt_counts, gt_flags), thresholds=thr)
    s = dict(det_boxes=boxes, det_counts=counts, gt_boxes=gt_boxes, gt_counts=gt_counts, gt_flags=gt_flags)
    ref = dsr.detect_score(s, C, thr)
    same(to_host(got), ref, "KerasYOLO.score")
    assert (ref["state"] == 1).any() and (ref["state"] == 0).any() and (ref["state"][0] != ref["state"][-1]).any()
    for method in dsr.METHODS:
        a = evaluate.average_precision(got, method)
        ap, maps, map_all = dsr.average_precision(ref, method)
        np.testing.assert_allclose(a["ap"], np.array(ap), rtol=1e-12, atol=0, equal_nan=True)
        np.testing.assert_allclose(a["map"], np.array(maps), rtol=1e-12, atol=0)
        np.testing.assert_allclose(a["map_all"], map_all, rtol=1e-12, atol=0)
    assert 0 < a["map_all"] < 1
    # numpy ground truth and device ground truth are the same call
    d = [dev(x, det.model.ctx) for x in (gt_boxes, gt_counts, gt_flags)]
    same(to_host(det.score(res, tuple(d), thresholds=thr)), ref, "device ground truth")
