"""GPU suite (-m gpu): HOTA scoring -- the alignment, the frames' weights and match, and the counts per IoU level on the device
("HOTA scoring").

Every device output is an integer and is compared bit for bit with the plain restatement tests/hota_score_ref.py: sizes, both tables,
align, w, dims, both ent arrays, the match, tp, loc and pairs.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import hota_score_ref as hsr
import identity_score_ref as isr
import track_score_ref as tsr

from test_gpu_track_memory import big_tracker, dev, small_tracker

pytestmark = pytest.mark.gpu

ARG = 1
ANY, RESUME = 1, 2
FILL = -7
_REF = {}


def ctx_():
    return small_tracker()[0].model.ctx


def on_dev(ctx, s, sl=slice(None)):
    """a scene dict (arrays without the clip axis) -> the six device tensors of one clip, frames sl"""
    return [dev(s[k][None, sl], ctx) for k in hsr.INPUTS]


def to_host(r, clip, T):
    """one clip of a Context.hota_score result -> the restatement's arrays (the match is [n * T, gcap] on the device)"""
    out = {k: r[k][clip].cpu().numpy() for k in hsr.ALL_KEYS if k != "row_to_col"}
    out["row_to_col"] = r["row_to_col"][clip * T:(clip + 1) * T].cpu().numpy()
    return out


def same(got, ref, what, keys=hsr.ALL_KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(ref[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


def gpu_score(ctx, s, any_label, acap, bcap, thresholds=hsr.THRESHOLDS, chunks=None):
    """one clip through Context.hota_align and Context.hota_score; chunks: both loops over chunks along T, through state= / align="""
    T = s["gt_boxes"].shape[0]
    if chunks is None:
        return to_host(ctx.hota_score(*on_dev(ctx, s), thresholds=thresholds, any_label=any_label, gt_cap=acap, hyp_cap=bcap), 0, T)
    al, t0 = None, 0
    for L in chunks:
        al = ctx.hota_align(*on_dev(ctx, s, slice(t0, t0 + L)), any_label=any_label, gt_cap=None if al else acap, hyp_cap=None if al else bcap,
                            state=al)
        t0 += L
    assert t0 == T
    parts, r, t0 = [], None, 0
    for L in chunks:
        r = ctx.hota_score(*on_dev(ctx, s, slice(t0, t0 + L)), thresholds=thresholds, align=al, state=r)
        parts.append(to_host(r, 0, L))
        t0 += L
    out = dict(parts[-1])
    for k in hsr.FRAME_KEYS:
        out[k] = np.concatenate([p[k] for p in parts])
    return out


def ref_score(key, s, any_label, acap, bcap, thresholds=hsr.THRESHOLDS):
    """the restatement, computed once per key"""
    if key not in _REF:
        _REF[key] = hsr.hota_score(*[s[k] for k in hsr.INPUTS], thresholds=thresholds, any_label=any_label, acap=acap, bcap=bcap)
    return _REF[key]


def wide_frame(gcap, hcap, T=2):
    """`gcap` ground-truth boxes in a row, `hcap` hypotheses jittered around them (every ground-truth box overlaps many), distinct ids"""
    rs = np.random.RandomState(gcap * 100 + hcap)
    s = dict(gt_boxes=np.zeros((T, gcap, 8), dtype=np.float32), gt_counts=np.full(T, gcap, dtype=np.int32),
             gt_ids=np.tile(np.arange(gcap, dtype=np.int32), (T, 1)), hyp_boxes=np.zeros((T, hcap, 8), dtype=np.float32),
             hyp_counts=np.full(T, hcap, dtype=np.int32), hyp_ids=np.tile(np.arange(hcap, dtype=np.int32)[::-1] + 7, (T, 1)).copy())
    lo = min(gcap, hcap)
    for t in range(T):
        for g in range(gcap):
            j = (rs.rand(2) - 0.5) * (0.1 if gcap > hcap else 0.0)
            s["gt_boxes"][t, g] = [0.2 + 0.3 * (g % lo) + j[0], 0.5 + j[1], 0.2, 0.3, 1.0, 0, 1.0, 0]
        for i in range(hcap):
            j = (rs.rand(2) - 0.5) * (0.1 if hcap > gcap else 0.0)
            s["hyp_boxes"][t, i] = [0.2 + 0.3 * (i % lo) + j[0], 0.5 + j[1], 0.2, 0.3, 0.9, 0, 0.8, 0]
    return s


# ------------------------------------------------------------------ 1. parity with the restatement
@pytest.mark.parametrize("any_label", [False, True])
@pytest.mark.parametrize("name", sorted(tsr.SCENES))
def test_parity_with_restatement(name, any_label):
    s, acap, bcap = isr.scene(name)
    ref = hsr.scene_ref(name, any_label)
    assert int(ref["tp"].sum()) > 0 and len(np.flatnonzero(ref["tp"])) > 3 and int(ref["align"].max()) > 0, "vacuous scene"
    assert int((ref["row_to_col"] >= 0).sum()) >= int(ref["tp"].sum())
    same(gpu_score(ctx_(), s, any_label, acap, bcap), ref, "%s, any_label %s" % (name, any_label))


def test_hand_example():
    h = hsr.hand_example()
    got = gpu_score(ctx_(), h, False, 4, 4)
    same(got, ref_score("hand", h, False, 4, 4), "hand example")
    S = hsr.S
    assert got["align"][:2, :2].tolist() == [[2 * S, 2 * S]] * 2 and got["tp"].tolist() == [0] * 18 + [8] and int(got["loc"][18]) == 8 * S
    assert got["w"][0, :2, :2].tolist() == [[1 + S // 3, 0], [0, 1 + S // 3]] and got["pairs"][18, :2, :2].tolist() == [[2, 2], [2, 2]]


# ------------------------------------------------------------------ 2. a frame wider than 64 lanes, and both solver orientations
@pytest.mark.parametrize("shape", [(3, 70), (70, 3)])
def test_wide_frame_and_its_transpose(shape):
    gcap, hcap = shape
    s = wide_frame(gcap, hcap)
    ref = ref_score(("wide_frame", shape), s, False, 80, 80)
    assert int((ref["w"][0] > 0).sum(axis=1 if hcap > gcap else 0).max()) > 10, "vacuous: a box must overlap many of the other side"
    assert int((ref["w"][0][:, 64:] > 0).sum() if hcap > 64 else (ref["w"][0][64:] > 0).sum()) > 0, "pairs beyond the first 64 lanes / rows"
    assert int((ref["row_to_col"] >= 0).sum()) == 2 * 3 and int(ref["tp"].sum()) == 6
    same(gpu_score(ctx_(), s, False, 80, 80), ref, "wide frame %s" % (shape,))


# ------------------------------------------------------------------ 3. edges: T = 1 and 5, empty frames, ids < 0, repeated ids, NaN boxes
def test_edge_clip():
    s = hsr.edge_clip()
    assert s["gt_counts"][1] == 0 and s["hyp_counts"][2] == 0 and (s["gt_ids"][0, :4] < 0).any() and (s["hyp_ids"][0, :5] < 0).any()
    assert len(set(s["gt_ids"][3, :4].tolist())) < 4 and len(set(s["hyp_ids"][3, :4].tolist())) < 4
    assert np.isnan(s["gt_boxes"][4, :3]).any() and np.isnan(s["hyp_boxes"][4, :4]).any()
    ctx = ctx_()
    for any_label in (False, True):
        ref = ref_score(("edge", any_label), s, any_label, 16, 16)
        assert ref["sizes"][7] > 10 and int(ref["tp"].sum()) > 5 and (ref["gt_ent"][4, :3] >= 0).all() and (ref["w"][4, 1] == 0).all()
        same(gpu_score(ctx, s, any_label, 16, 16), ref, "edge clip, any_label %s" % any_label)
    one = {k: v[:1] for k, v in s.items()}
    same(gpu_score(ctx, one, False, 16, 16), ref_score("edge_T1", one, False, 16, 16), "T = 1")


def test_table_overflow_on_each_side():
    ctx = ctx_()
    s = hsr.edge_clip()
    for ac, bc in ((2, 16), (16, 2), (2, 2)):
        ref = ref_score(("edge_caps", ac, bc), s, False, ac, bc)
        assert (ref["sizes"][5] > 0) == (ac == 2) and (ref["sizes"][6] > 0) == (bc == 2) and ref["sizes"][7] > 0
        assert ref["sizes"][3] == min(ac, 5) and (ref["gt_ent"].max() < ac) and (ref["hyp_ent"].max() < bc)
        same(gpu_score(ctx, s, False, ac, bc), ref, "acap %d, bcap %d" % (ac, bc))


# ------------------------------------------------------------------ 4. thresholds: one, nineteen, and one equal to a pair's IoU
def test_thresholds_one_and_equal_to_an_iou():
    ctx = ctx_()
    s = hsr.edge_clip()
    iou = np.float32(hsr.orc.bbox_iou(s["gt_boxes"][0, 3, :4], s["hyp_boxes"][0, 3, :4]))
    assert 0.45 < iou < 0.55
    full = ref_score(("edge", False), s, False, 16, 16)
    assert full["row_to_col"][0, 3] == 3, "the pair is matched"
    above = np.nextafter(iou, np.float32(1))
    counts = []
    for name, thr in (("one", [0.5]), ("at", [iou]), ("above", [above]), ("both", [iou, above])):
        ref = ref_score(("edge_thr", name), s, False, 16, 16, thresholds=np.array(thr, dtype=np.float32))
        got = gpu_score(ctx, s, False, 16, 16, thresholds=thr)
        same(got, ref, "thresholds %s" % name)
        assert got["tp"].shape == (len(thr),) and got["pairs"].shape == (len(thr), 16, 16)
        counts.append(got["tp"].tolist())
    assert counts[1][0] == counts[2][0] + 1, "IoU >= threshold: the pair counts at its own IoU and not one ulp above"
    assert counts[3] == [1, counts[2][0]], "bucket 0 holds the pairs that reach the first threshold only"


# ------------------------------------------------------------------ 5. the tables are identity scoring's
def test_tables_equal_identity_overlap_on_the_device():
    ctx = ctx_()
    for name in ("small", "repeated_ids"):
        s, acap, bcap = isr.scene(name)
        d = on_dev(ctx, s)
        al = ctx.hota_align(*d, gt_cap=acap, hyp_cap=bcap)
        idn = ctx.identity_overlap(*d, gt_cap=acap, hyp_cap=bcap)
        assert torch.equal(al["sizes"][:, :7], idn["sizes"][:, :7]) and torch.equal(al["gt_tab"], idn["gt_tab"])
        assert torch.equal(al["hyp_tab"], idn["hyp_tab"]) and al["align"].dtype == torch.int64


# ------------------------------------------------------------------ 6. the chunk contract
def test_chunks_equal_one_call():
    ctx = ctx_()
    s = hsr.edge_clip()
    ref = ref_score(("edge", False), s, False, 16, 16)
    same(gpu_score(ctx, s, False, 16, 16, chunks=[1, 3, 1]), ref, "chunks (1, 3, 1)")
    # vacuity: the counts of the last chunk alone differ, and so do its weights under the alignment of that chunk alone
    tail = gpu_score(ctx, {k: v[4:] for k, v in s.items()}, False, 16, 16)
    assert not np.array_equal(tail["tp"], ref["tp"]) and not np.array_equal(tail["w"][0], ref["w"][4])


# ------------------------------------------------------------------ 7. the C entries: uninitialised buffers, errors
def raw_call(ctx, name, a):
    import mi355_dt
    p = lambda x: mi355_dt._dptr(x) if x is None or torch.is_tensor(x) else x
    ctx._sync_stream()
    rc = getattr(ctx.lib, name)(ctx.h, *[p(v) for v in a.values()])
    torch.cuda.synchronize()
    return rc


def raw_buffers(ctx, d, acap, bcap, n_thr):
    n, T, gcap, _ = d[0].shape
    hcap = d[3].shape[2]
    full = lambda dt, *s: torch.full(s, FILL, dtype=dt, device=ctx.device)
    i32, i64 = torch.int32, torch.int64
    return dict(sizes=full(i32, n, 8), gt_tab=full(i32, n, acap, 2), hyp_tab=full(i32, n, bcap, 2), align=full(i64, n, acap, bcap),
                w=full(i32, n, T, gcap, hcap), dims=full(i32, n, T, 2), gt_ent=full(i32, n, T, gcap), hyp_ent=full(i32, n, T, hcap),
                tp=full(i32, n, n_thr), loc=full(i64, n, n_thr), pairs=full(i32, n, n_thr, acap, bcap))


def args_of(d, o, acap, bcap, thr, r2c=None):
    """the three entries' arguments, in the order of the declarations"""
    n, T, gcap, _ = d[0].shape
    hcap = d[3].shape[2]
    lead = dict(gt_boxes=d[0], gt_counts=d[1], gt_ids=d[2], gcap=gcap, hyp_boxes=d[3], hyp_counts=d[4], hyp_ids=d[5], hcap=hcap, id_stride=1,
                label_at=5, n=n, T=T, flags=0, acap=acap, bcap=bcap)
    align = dict(lead, sizes=o["sizes"], gt_tab=o["gt_tab"], hyp_tab=o["hyp_tab"], align=o["align"])
    weights = dict(align, w=o["w"], dims=o["dims"], gt_ent=o["gt_ent"], hyp_ent=o["hyp_ent"])
    count = dict(gt_boxes=d[0], gcap=gcap, hyp_boxes=d[3], hcap=hcap, n=n, T=T, dims=o["dims"], gt_ent=o["gt_ent"], hyp_ent=o["hyp_ent"],
                 r2c=r2c, thr=thr.ctypes.data_as(ctypes.c_void_p), n_thr=len(thr), acap=acap, bcap=bcap, flags=0, tp=o["tp"], loc=o["loc"],
                 pairs=o["pairs"])
    return align, weights, count


def untouched(o, keys):
    return all(bool((o[k] == FILL).all()) for k in keys)


def test_uninitialised_outputs_are_fully_written_and_errors_leave_them_untouched():
    ctx = ctx_()
    s = hsr.edge_clip()
    acap = bcap = 16
    ref = ref_score(("edge", False), s, False, acap, bcap)
    d = on_dev(ctx, s)
    thr = np.ascontiguousarray(hsr.THRESHOLDS)
    gcap, hcap = d[0].shape[2], d[3].shape[2]
    OUT_A, OUT_W, OUT_C = hsr.ALIGN_KEYS, ("w", "dims", "gt_ent", "hyp_ent"), hsr.COUNT_KEYS

    # every output pre-filled with -7, no RESUME: every word is written
    o = raw_buffers(ctx, d, acap, bcap, len(thr))
    a, w, c = args_of(d, o, acap, bcap, thr)
    assert raw_call(ctx, "dt_hota_align", a) == 0 and raw_call(ctx, "dt_hota_weights", w) == 0
    r2c, _, _ = ctx.assign_max(o["w"].view(-1, gcap, hcap), o["dims"].view(-1, 2))
    c["r2c"] = r2c
    assert raw_call(ctx, "dt_hota_count", c) == 0
    got = {k: o[k][0].cpu().numpy() for k in OUT_A + OUT_W + OUT_C}
    got["row_to_col"] = r2c.cpu().numpy()
    same(got, ref, "buffers pre-filled with -7")
    good = {k: v.clone() for k, v in o.items()}

    # the alignment's errors
    fits = (40960 - 2 * bcap - 9 * gcap - 9 * hcap) // 2
    bad = [dict(gt_boxes=None), dict(gt_counts=None), dict(gt_ids=None), dict(hyp_boxes=None), dict(hyp_counts=None), dict(hyp_ids=None),
           dict(sizes=None), dict(gt_tab=None), dict(hyp_tab=None), dict(align=None), dict(n=-1), dict(T=0), dict(T=-3), dict(gcap=0),
           dict(hcap=0), dict(hcap=-1), dict(acap=0), dict(acap=-2), dict(bcap=0), dict(bcap=-1), dict(id_stride=0), dict(label_at=-1),
           dict(label_at=8), dict(flags=4), dict(flags=8 | ANY), dict(flags=-1), dict(acap=fits + 1), dict(n=1 << 19, acap=64, bcap=64)]
    o = raw_buffers(ctx, d, acap, bcap, len(thr))
    a, w, c = args_of(d, o, acap, bcap, thr, r2c)
    for over in bad:
        assert raw_call(ctx, "dt_hota_align", dict(a, **over)) == ARG and untouched(o, OUT_A), over
    assert raw_call(ctx, "dt_hota_align", dict(a, n=0)) == 0 and untouched(o, OUT_A), "n_clips = 0 is a no-op"

    # the weights': the inputs are the finished alignment
    for k in OUT_A:
        w[k] = good[k]
    fits = (40960 - 2 * bcap - 7 * gcap - 7 * hcap) // 2
    bad = bad[:6] + [dict(sizes=None), dict(gt_tab=None), dict(hyp_tab=None), dict(align=None), dict(w=None), dict(dims=None),
                     dict(gt_ent=None), dict(hyp_ent=None)] + bad[10:23] + \
        [dict(flags=RESUME), dict(flags=4), dict(flags=-1), dict(acap=fits + 1), dict(n=1 << 19, acap=64, bcap=64), dict(n=1 << 25, acap=4, bcap=4)]
    for over in bad:
        assert raw_call(ctx, "dt_hota_weights", dict(w, **over)) == ARG and untouched(o, OUT_W), over
    assert raw_call(ctx, "dt_hota_weights", dict(w, n=0)) == 0 and untouched(o, OUT_W)

    # the count's
    for k in OUT_W:
        c[k] = good[k]
    host = lambda *v: np.array(v, dtype=np.float32)
    thr_bad = [host(0.5, 0.5), host(0.6, 0.5), host(0.0, 0.5), host(-0.1), host(1.5), host(0.5, float("nan")), host(float("nan")),
               host(0.5, float("inf"))]
    bad = [dict(gt_boxes=None), dict(hyp_boxes=None), dict(dims=None), dict(gt_ent=None), dict(hyp_ent=None), dict(r2c=None), dict(thr=None),
           dict(tp=None), dict(loc=None), dict(pairs=None), dict(n=-1), dict(T=0), dict(gcap=0), dict(hcap=-1), dict(acap=0), dict(bcap=-2),
           dict(n_thr=0), dict(n_thr=-1), dict(n_thr=33), dict(flags=ANY), dict(flags=4), dict(flags=-1), dict(n=1 << 15, acap=64, bcap=64),
           dict(n=1 << 28)]
    bad += [dict(thr=t.ctypes.data_as(ctypes.c_void_p), n_thr=len(t)) for t in thr_bad]
    for over in bad:
        assert raw_call(ctx, "dt_hota_count", dict(c, **over)) == ARG and untouched(o, OUT_C), over
    assert raw_call(ctx, "dt_hota_count", dict(c, n=0)) == 0 and untouched(o, OUT_C)
    with pytest.raises(Exception):
        ctx.hota_score(*d, thresholds=[0.5, 0.5], gt_cap=acap, hyp_cap=bcap)

    # following valid calls are unaffected, and RESUME adds to the counts
    assert raw_call(ctx, "dt_hota_count", c) == 0
    same({k: o[k][0].cpu().numpy() for k in OUT_C}, ref, "after the refused calls", OUT_C)
    assert raw_call(ctx, "dt_hota_count", dict(c, flags=RESUME)) == 0
    for k in OUT_C:
        assert np.array_equal(o[k][0].cpu().numpy(), 2 * ref[k]), k


# ------------------------------------------------------------------ 8. several clips in one call
def test_three_clips_in_one_call_equal_three_calls():
    ctx = ctx_()
    base = hsr.edge_clip()
    clips = [base, {k: v[::-1].copy() for k, v in base.items()}, {k: np.roll(v, 2, axis=0) for k, v in base.items()}]
    refs = [ref_score(("edge3", k), s, False, 16, 16) for k, s in enumerate(clips)]
    assert len({r["tp"].tobytes() + r["align"].tobytes() for r in refs}) == 3, "the clips must differ"
    d = [dev(np.stack([s[k] for s in clips]), ctx) for k in hsr.INPUTS]
    got = ctx.hota_score(*d, gt_cap=16, hyp_cap=16)
    for k, s in enumerate(clips):
        one = to_host(got, k, 5)
        same(one, refs[k], "clip %d of three" % k)
        same(gpu_score(ctx, s, False, 16, 16), one, "clip %d alone" % k)


# ------------------------------------------------------------------ 9. the tracker's own method, on its own result
def test_tracker_hota_on_a_track_clips_result():
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
        plain = trk.hota(res, gt)
        ctx.profile_enable(False)
        for name in ("score:hota_align", "score:hota_weights", "associate:assign_max", "score:hota_count"):
            assert name in ctx.profile_names(), name
        p = evaluate.hota(plain)["pooled"]
        assert (p["gt"], p["hyp"], p["overflow"]) == (total, total, 0) and p["TP"].tolist() == [total] * 19
        for k in ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr"):
            assert (p[k] == 1.0).all(), k
        assert p["hota"] == 1.0 and p["hota0"] == 1.0 and (p["LocA"] >= 1.0 - 2.0 ** -20).all() and (p["LocA"] <= 1.0).all()
        assert p["gt_tracks"] == p["hyp_tracks"] == int(res["nids"].sum())
        # the confirmed-track read-out of the same boxes as hypotheses
        with pytest.raises(Exception):
            trk.hota(res, gt, confirmed=True)
        a = ctx.associate_tracks(res["boxes"], res["counts"], trk.ASSOC_THRESHOLD, 2, 0.5, 2, track_cap=cap)
        conf = trk.hota(dict(res, tracks=a["tracks"], track_counts=a["track_counts"], track_info=a["track_info"]), gt, confirmed=True,
                        thresholds=[0.5, 0.75])
        k = 0                                                    # one clip against the restatement: the label is float 4, the id word 0 of 4
        ref = hsr.hota_score(*[x[k].cpu().numpy() for x in gt], a["tracks"][k].cpu().numpy(), a["track_counts"][k].cpu().numpy(),
                             a["track_info"][k].cpu().numpy(), thresholds=[0.5, 0.75], acap=int(conf["gt_tab"].shape[1]),
                             bcap=int(conf["hyp_tab"].shape[1]), label_at=4)
        same(to_host(conf, k, T), ref, "confirmed, clip %d" % k)
        q = evaluate.hota(conf)["pooled"]
        assert q["hyp"] != p["hyp"] and 0 < q["TP"][0] < total and 0.0 < q["hota"] < 1.0, "vacuous: the read-out scores as the boxes do"


# ------------------------------------------------------------------ 10. the library exports the entries
def test_library_exports_the_entries():
    import mi355_dt
    out = subprocess.run(["nm", "-D", "--defined-only", mi355_dt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("dt_hota_align", "dt_hota_weights", "dt_hota_count"):
        assert name in exported and name in mi355_dt.SYMBOLS
    assert ctx_().lib.dt_abi_version() == 108
