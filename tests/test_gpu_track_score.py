"""GPU suite (-m gpu): track scoring -- CLEAR-MOT counts against ground-truth tracks on the device.

Every integer output is compared exactly with the plain restatement tests/track_score_ref.py, and `miou` through an int32 view:
the IoU keys are compared as bits in the kernel and score.hip forms no fused multiply-add.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import track_score_ref as tsr

from test_gpu_track_memory import big_tracker, dev, small_tracker

pytestmark = pytest.mark.gpu

ARG = 1
ANY, RESUME = 1, 2
INPUTS = ("gt_boxes", "gt_counts", "gt_ids", "hyp_boxes", "hyp_counts", "hyp_ids")
_REF = {}


def ctx_():
    return small_tracker()[0].model.ctx


def on_dev(ctx, s, sl=slice(None)):
    """a scene dict (arrays without the clip axis) -> the six device tensors of one clip, frames sl"""
    return [dev(s[k][None, sl], ctx) for k in INPUTS]


def to_host(r, clip=0):
    out = {k: (r[k][clip].cpu().numpy() if r[k] is not None else None) for k in tsr.KEYS}
    out["nobjs"] = int(out["nobjs"])
    return out


def same(got, ref, what):
    for k in tsr.KEYS:
        if got[k] is None:
            continue
        g, w = np.asarray(got[k]), np.asarray(ref[k])
        if k == "miou":
            g, w = g.view(np.int32), w.view(np.int32)
        assert g.shape == w.shape and np.array_equal(g, w), (what, k)


def gpu_score(ctx, s, any_label, ocap, chunks=None, resume=True):
    """one clip through Context.track_score, in chunks along T through `state` (resume=False: the state is dropped)"""
    T = s["gt_boxes"].shape[0]
    parts, t0, state = [], 0, None
    for L in (chunks or [T]):
        r = ctx.track_score(*on_dev(ctx, s, slice(t0, t0 + L)), iou_threshold=0.5, any_label=any_label, obj_cap=ocap, state=state)
        state = r if resume else None
        parts.append(to_host(r))
        t0 += L
    assert t0 == T
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("frame_counts", "match", "miou")}
    out.update({k: parts[-1][k] for k in ("totals", "objs", "nobjs")})
    return out


def raw_score(ctx, d, ocap, flags=0, thr=0.5, fcounts=True, match=True, miou=True, fill=-7, **over):
    """the C entry on the six device tensors d, every output pre-filled; `over` replaces arguments by name -> (return code, outputs)"""
    import mi355_dt
    n, T, gcap, _ = d[0].shape
    hcap = d[3].shape[2]
    i32 = lambda *s: torch.full(s, fill, dtype=torch.int32, device=ctx.device)
    o = dict(totals=i32(n, 8), objs=i32(n, max(ocap, 1), 8), nobjs=i32(n), frame_counts=i32(n, T, 4) if fcounts else None,
             match=i32(n, T, gcap) if match else None, miou=torch.full((n, T, gcap), float(fill), device=ctx.device) if miou else None)
    a = dict(gt_boxes=d[0], gt_counts=d[1], gt_ids=d[2], gcap=gcap, hyp_boxes=d[3], hyp_counts=d[4], hyp_ids=d[5], hcap=hcap, id_stride=1,
             label_at=5, n=n, T=T, thr=thr, flags=flags, ocap=ocap, totals=o["totals"], objs=o["objs"], nobjs=o["nobjs"])
    a.update(over)
    p = lambda x: mi355_dt._dptr(x) if x is None or torch.is_tensor(x) else x
    ctx._sync_stream()
    rc = ctx.lib.dt_track_score(ctx.h, p(a["gt_boxes"]), p(a["gt_counts"]), p(a["gt_ids"]), a["gcap"], p(a["hyp_boxes"]), p(a["hyp_counts"]),
                                p(a["hyp_ids"]), a["hcap"], a["id_stride"], a["label_at"], a["n"], a["T"], a["thr"], a["flags"], a["ocap"],
                                p(a["totals"]), p(a["objs"]), p(a["nobjs"]), p(o["frame_counts"]), p(o["match"]), p(o["miou"]))
    torch.cuda.synchronize()
    return rc, o


def untouched(o, fill=-7):
    return all(bool((v.view(torch.int32) == (torch.tensor(float(fill)).view(torch.int32).item() if v.dtype == torch.float32 else fill)).all())
               for v in o.values() if v is not None)


# ------------------------------------------------------------------ 1. parity with the restatement
@pytest.mark.parametrize("any_label", [False, True])
@pytest.mark.parametrize("name", sorted(tsr.SCENES))
def test_parity_with_restatement(name, any_label):
    s, ocap = tsr.scene(name)
    ref = tsr.scene_ref(name, any_label)
    m, f, sw = tsr.misses_fps_switches(ref)
    assert m > 0 and f > 0 and sw > 0, "vacuous scene"
    if name == "wide":
        assert s["gt_boxes"].shape[1] > 64 and s["hyp_boxes"].shape[1] > 128 and ref["nobjs"] > 128
    same(gpu_score(ctx_(), s, any_label, ocap), ref, "%s, any_label %s" % (name, any_label))


# ------------------------------------------------------------------ 2. the worked example
def test_worked_example():
    got = gpu_score(ctx_(), tsr.worked_example(), False, 4)
    assert got["totals"].tolist() == tsr.WORKED_TOTALS
    assert got["nobjs"] == 1 and got["objs"][0].tolist() == tsr.WORKED_OBJ
    assert got["objs"][1:].tolist() == [[-1, -1, 0, 0, 0, 0, 0, 0]] * 3
    assert got["match"][:, 0].tolist() == tsr.WORKED_MATCH and (got["match"][:, 1] == -1).all()
    assert got["frame_counts"].tolist() == tsr.WORKED_FRAME_COUNTS
    same(got, tsr.track_score(thr=0.5, ocap=4, **tsr.worked_example()), "worked example")


def test_an_id_in_two_rows_of_a_frame():
    """the hand-made frames tests/test_track_score_cpu.py asserts on the restatement: the lower row matched and the higher not, and the reverse"""
    for matched_row, first, second in ((0, [9, 5, 2, 1, 0, 0, 0, 0], [9, 6, 3, 2, 1, 1, 1, 0]),
                                       (1, [9, 5, 2, 1, 0, 0, 1, 0], [9, 6, 3, 2, 1, 0, 1, 0])):
        s = tsr.two_rows(matched_row)
        head = {k: s[k][:1] for k in INPUTS}
        assert gpu_score(ctx_(), head, False, 4)["objs"][0].tolist() == first, matched_row
        got = gpu_score(ctx_(), s, False, 4)
        assert got["objs"][0].tolist() == second, matched_row
        same(got, tsr.track_score(*(s[k] for k in INPUTS), 0.5, False, 4), "an id in two rows, row %d matched" % matched_row)


def test_repeated_ids_scene_covers_the_orders():
    """the parity scene `repeated_ids` holds, per the restatement, both orders of matched and unmatched rows of one id, such rows in
    different 64-row passes, matched rows with id < 0 and hypotheses that share an id"""
    s, _ = tsr.scene("repeated_ids")
    assert min(tsr.repeated_id_cases(s, tsr.scene_ref("repeated_ids", False))) > 0


# ------------------------------------------------------------------ 3. a full object table
def test_overflow():
    if "overflow" not in _REF:
        s = tsr.make_scene(20, 32, 32, 30, 7)
        args = [s[k] for k in INPUTS]
        _REF["overflow"] = (s, tsr.track_score(*args, 0.5, False, 16), tsr.track_score(*args, 0.5, False, 64))
    s, tight, roomy = _REF["overflow"]
    assert tight["totals"][6] > 0 and tight["nobjs"] == 16 and roomy["totals"][6] == 0 and roomy["nobjs"] > 16
    g16, g64 = gpu_score(ctx_(), s, False, 16), gpu_score(ctx_(), s, False, 64)
    same(g16, tight, "ocap 16")
    same(g64, roomy, "ocap 64")
    agree = (tight["objs"][:16] == roomy["objs"][:16]).all(axis=1)
    assert agree.any()
    assert np.array_equal(g16["objs"][:16][agree], g64["objs"][:16][agree])


# ------------------------------------------------------------------ 4. the confirmed-track read-out as hypotheses
def test_readout_form():
    trk = small_tracker()[0]
    ctx = trk.model.ctx
    s, ocap = tsr.scene("small")
    d = on_dev(ctx, s)
    a = ctx.associate_tracks(d[3], d[4], 0.3, 3, 0.5, 2, track_cap=48)
    assert tuple(a["track_info"].shape[2:]) == (48, 4) and int((a["track_info"][..., 1] > 0).sum()) > 0, "no coasting row"
    got = to_host(ctx.track_score(d[0], d[1], d[2], a["tracks"], a["track_counts"], a["track_info"], obj_cap=ocap))
    ref = tsr.track_score(s["gt_boxes"], s["gt_counts"], s["gt_ids"], a["tracks"][0].cpu().numpy(), a["track_counts"][0].cpu().numpy(),
                          a["track_info"][0].cpu().numpy(), 0.5, False, ocap, label_at=4)
    same(got, ref, "read-out form")
    by_boxes = to_host(ctx.track_score(d[0], d[1], d[2], d[3], d[4], a["ids"], obj_cap=ocap))
    assert not np.array_equal(by_boxes["totals"], got["totals"]), "vacuous: the read-out scores as the boxes do"
    # ... and through the tracker's own method
    res = dict(a, boxes=d[3], counts=d[4])
    gt = (s["gt_boxes"][None], s["gt_counts"][None], s["gt_ids"][None])
    same(to_host(trk.score(res, gt, confirmed=True, obj_cap=ocap)), ref, "MultiObjDetTracker.score, confirmed")
    same(to_host(trk.score(res, gt, obj_cap=ocap)), by_boxes, "MultiObjDetTracker.score")


# ------------------------------------------------------------------ 5. many clips in one call
def test_48_clips_in_one_call():
    """one wavefront per clip: 48 clips of different seeds in one launch, each equal to its own single-clip restatement"""
    ctx = ctx_()
    T, cap, ocap = 30, 16, 64
    if "clips48" not in _REF:
        scenes = [tsr.make_scene(T, cap, cap, 6 + k % 5, 100 + k) for k in range(48)]
        refs = [tsr.track_score(*[s[k] for k in INPUTS], 0.5, False, ocap) for s in scenes]
        _REF["clips48"] = (scenes, refs)
    scenes, refs = _REF["clips48"]
    d = [dev(np.stack([s[k] for s in scenes]), ctx) for k in INPUTS]
    got = ctx.track_score(*d, obj_cap=ocap)
    for k in range(48):
        same(to_host(got, k), refs[k], "clip %d" % k)
    assert len(set(tuple(r["totals"]) for r in refs)) > 40, "the clips must differ"


# ------------------------------------------------------------------ 6. resume
@pytest.mark.parametrize("name", ["small", "long"])
def test_resume_chunks_equal_one_call(name):
    ctx = ctx_()
    s, ocap = tsr.scene(name)
    T = s["gt_boxes"].shape[0]
    whole = gpu_score(ctx, s, False, ocap)
    same(whole, tsr.scene_ref(name, False), name)
    for chunks in ([1, 7, T - 8], [T - 1, 1]):
        same(gpu_score(ctx, s, False, ocap, chunks=chunks), whole, "%s in chunks %s" % (name, chunks))
    dropped = gpu_score(ctx, s, False, ocap, chunks=[8, T - 8], resume=False)
    assert not np.array_equal(dropped["totals"], whole["totals"]) and not np.array_equal(dropped["frame_counts"], whole["frame_counts"]), \
        "vacuous: the second chunk does not depend on the state"


# ------------------------------------------------------------------ 7. uninitialised output buffers
def test_uninitialised_outputs_are_fully_written():
    ctx = ctx_()
    s, ocap = tsr.scene("small")
    ref = tsr.scene_ref("small", False)
    for fill in (-7, 0x55555555):
        rc, o = raw_score(ctx, on_dev(ctx, s), ocap, fill=fill)
        assert rc == 0
        same(to_host(o), ref, "buffers pre-filled with %d" % fill)


# ------------------------------------------------------------------ 8. optional outputs NULL
def test_optional_outputs_null():
    ctx = ctx_()
    s, ocap = tsr.scene("small")
    ref = tsr.scene_ref("small", False)
    d = on_dev(ctx, s)
    for off in (dict(fcounts=False), dict(match=False, miou=False), dict(fcounts=False, match=False, miou=False)):
        rc, o = raw_score(ctx, d, ocap, **off)
        assert rc == 0, off
        same(to_host(o), ref, off)
    lean = ctx.track_score(*d, obj_cap=ocap, per_box=False)
    assert lean["match"] is None and lean["miou"] is None
    same(to_host(lean), ref, "per_box=False")


# ------------------------------------------------------------------ 9. errors
def test_errors_leave_the_outputs_untouched():
    ctx = ctx_()
    s, ocap = tsr.scene("small")
    ref = tsr.scene_ref("small", False)
    d = on_dev(ctx, s)
    gcap, hcap = d[0].shape[2], d[3].shape[2]
    words = lambda oc: 8 * oc + 11 * gcap + 7 * hcap
    fits = (40960 - 11 * gcap - 7 * hcap) // 8
    assert words(fits) <= 40960 < words(fits + 1)
    bad = [dict(gt_boxes=None), dict(gt_counts=None), dict(gt_ids=None), dict(hyp_boxes=None), dict(hyp_counts=None), dict(hyp_ids=None),
           dict(totals=None), dict(objs=None), dict(nobjs=None),
           dict(n=-1), dict(T=0), dict(T=-3), dict(gcap=0), dict(hcap=0), dict(hcap=-1), dict(ocap=0), dict(ocap=-2), dict(id_stride=0),
           dict(label_at=-1), dict(label_at=8), dict(flags=4), dict(flags=8 | ANY), dict(flags=-1),
           dict(thr=float("nan")), dict(thr=0.0), dict(thr=-0.1), dict(thr=1.5), dict(thr=float("inf")), dict(ocap=fits + 1)]
    for over in bad:
        kw = dict(over)
        rc, o = raw_score(ctx, d, kw.pop("ocap", ocap), **kw)
        assert rc == ARG and untouched(o), over
    for off in (dict(match=False), dict(miou=False)):
        rc, o = raw_score(ctx, d, ocap, **off)
        assert rc == ARG and untouched(o), off
    rc, o = raw_score(ctx, d, ocap, n=0)
    assert rc == 0 and untouched(o), "n_clips = 0 is a no-op"
    with pytest.raises(Exception):
        ctx.track_score(*d, iou_threshold=0.0, obj_cap=ocap)
    # a following valid call is unaffected -- and the largest table that fits the LDS launches
    rc, o = raw_score(ctx, d, ocap)
    assert rc == 0
    same(to_host(o), ref, "after the refused calls")
    rc, o = raw_score(ctx, d, fits, thr=1.0)
    assert rc == 0
    got = to_host(o)
    assert got["nobjs"] == ref["nobjs"] and (got["objs"][ref["nobjs"]:] == [-1, -1, 0, 0, 0, 0, 0, 0]).all()
    assert got["totals"][1] == ref["totals"][1] and got["totals"][3] < ref["totals"][3], "threshold 1 keeps fewer pairs"


# ------------------------------------------------------------------ 10. the library exports the entry
def test_library_exports_the_entry():
    import mi355_dt
    out = subprocess.run(["nm", "-D", "--defined-only", mi355_dt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "dt_track_score" in exported and "dt_track_score" in mi355_dt.SYMBOLS
    header = open(os.path.join(os.path.dirname(mi355_dt.LIB_PATH), "..", "include", "mi355_dt.h")).read()
    assert "dt_track_score(" in header
    assert (mi355_dt.DT_SCORE_ANY_LABEL, mi355_dt.DT_SCORE_RESUME, mi355_dt.DT_SCORE_INTS, mi355_dt.DT_SCORE_OBJ_INTS) == (ANY, RESUME, 8, 8)
    assert ctx_().lib.dt_abi_version() == 108


# ------------------------------------------------------------------ 11. end to end at 416
def test_end_to_end_416():
    from parallel import pinned_policy
    from utility import evaluate
    trk, blob, tw, fr = big_tracker()
    ctx = trk.model.ctx
    with pinned_policy(ctx):
        res = trk.track_clips(fr)
        n, T, cap = res["ids"].shape
        total = int(torch.minimum(res["counts"], torch.tensor(cap, device=ctx.device)).sum())
        assert (n, T) == (2, 30) and total > 0
        gt = (res["boxes"], res["counts"], res["ids"])
        ctx.profile_reset(); ctx.profile_enable(True)
        sc = trk.score(res, gt)
        ctx.profile_enable(False)
        assert "associate:score" in ctx.profile_names()
        p = evaluate.summarize(sc)["pooled"]
        assert (p["gt"], p["hyp"], p["matches"]) == (total, total, total)
        assert (p["misses"], p["false_positives"], p["switches"], p["fragments"], p["overflow"]) == (0, 0, 0, 0, 0)
        assert p["mota"] == 1.0 and p["motp"] > 0.999 and p["objects"] == int(res["nids"].sum())
        for k in range(n):
            objs = sc["objs"][k, :int(sc["nobjs"][k])].cpu().numpy()
            assert (objs[:, 0] == objs[:, 1]).all() and (objs[:, 2] == objs[:, 3]).all()
        # the ground-truth ids one frame late: the same boxes now change their object from frame to frame
        late = torch.roll(res["ids"], 1, dims=1).contiguous()
        p2 = evaluate.summarize(trk.score(res, (res["boxes"], res["counts"], late)))["pooled"]
        assert p2["switches"] > 0 and p2["gt"] == total
