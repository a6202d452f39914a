"""GPU suite (-m gpu): identity scoring -- the trajectory overlap and the optimal assignment on the device.

Every output is an integer and is compared exactly with the plain restatement tests/identity_score_ref.py, the assignment itself
included: the solver's steps are stated in DESIGN.md, and the IoU comparison is the one track scoring's tests pin bit for bit.
"""
import subprocess

import numpy as np
import pytest
import torch

import identity_score_ref as isr
import track_score_ref as tsr

from test_gpu_track_memory import big_tracker, dev, small_tracker

pytestmark = pytest.mark.gpu

ARG = 1
ANY, RESUME = 1, 2
_REF = {}


def ctx_():
    return small_tracker()[0].model.ctx


def on_dev(ctx, s, sl=slice(None)):
    """a scene dict (arrays without the clip axis) -> the six device tensors of one clip, frames sl"""
    return [dev(s[k][None, sl], ctx) for k in isr.INPUTS]


def to_host(r, clip=0, keys=isr.ALL_KEYS):
    return {k: r[k][clip].cpu().numpy() for k in keys if k in r}


def same(got, ref, what, keys=isr.ALL_KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(ref[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


def gpu_score(ctx, s, any_label, acap, bcap, chunks=None, resume=True):
    """one clip through Context.identity_score, in chunks along T through `state` (resume=False: the state is dropped)"""
    T = s["gt_boxes"].shape[0]
    t0, state, r = 0, None, None
    for L in (chunks or [T]):
        r = ctx.identity_score(*on_dev(ctx, s, slice(t0, t0 + L)), iou_threshold=0.5, any_label=any_label, gt_cap=acap, hyp_cap=bcap,
                               state=state)
        state = r if resume else None
        t0 += L
    assert t0 == T
    return to_host(r)


def gpu_assign(ctx, mats, rcap=None, ccap=None, dims_stride=None):
    """problems of different sizes in one dt_assign_max call, each in the corner of a [rcap, ccap] block whose rest is filled with a
    weight that would win if it were read -> list of (row_to_col, col_to_row, total) on the host"""
    rcap = rcap or max(m.shape[0] for m in mats)
    ccap = ccap or max(m.shape[1] for m in mats)
    w = np.full((len(mats), rcap, ccap), 1 << 20, dtype=np.int32)
    stride, ra, ca = (dims_stride, 3, 4) if dims_stride else (2, 0, 1)
    dims = np.full((len(mats), stride), -9, dtype=np.int32)
    for k, m in enumerate(mats):
        w[k, :m.shape[0], :m.shape[1]] = m
        dims[k, ra], dims[k, ca] = m.shape
    r2c, c2r, total = ctx.assign_max(dev(w, ctx), dev(dims, ctx), ra, ca)
    assert r2c.dtype == torch.int32 and c2r.dtype == torch.int32 and total.dtype == torch.int64
    r2c, c2r, total = r2c.cpu().numpy(), c2r.cpu().numpy(), total.cpu().numpy()
    return [(r2c[k], c2r[k], int(total[k])) for k in range(len(mats))]


def ref_assign(m, rcap, ccap):
    w = np.zeros((rcap, ccap), dtype=np.int64)
    w[:m.shape[0], :m.shape[1]] = m
    return isr.assign_max(w, m.shape[0], m.shape[1])


def raw_overlap(ctx, d, rows_a, rows_b, flags=0, thr=0.5, fill=-7, **over):
    """the C entry on the six device tensors d, every output pre-filled, the tables with rows_a / rows_b rows; `over` replaces
    arguments by name (acap, bcap too: the buffers keep their sizes) -> (return code, outputs)"""
    acap, bcap = rows_a, rows_b
    import mi355_dt
    n, T, gcap, _ = d[0].shape
    hcap = d[3].shape[2]
    i32 = lambda *s: torch.full(s, fill, dtype=torch.int32, device=ctx.device)
    o = dict(sizes=i32(n, 8), gt_tab=i32(n, max(acap, 1), 2), hyp_tab=i32(n, max(bcap, 1), 2), overlap=i32(n, max(acap, 1), max(bcap, 1)))
    a = dict(gt_boxes=d[0], gt_counts=d[1], gt_ids=d[2], gcap=gcap, hyp_boxes=d[3], hyp_counts=d[4], hyp_ids=d[5], hcap=hcap, id_stride=1,
             label_at=5, n=n, T=T, thr=thr, flags=flags, acap=acap, bcap=bcap)
    a.update(o)
    a.update(over)
    p = lambda x: mi355_dt._dptr(x) if x is None or torch.is_tensor(x) else x
    ctx._sync_stream()
    rc = ctx.lib.dt_identity_overlap(ctx.h, p(a["gt_boxes"]), p(a["gt_counts"]), p(a["gt_ids"]), a["gcap"], p(a["hyp_boxes"]),
                                     p(a["hyp_counts"]), p(a["hyp_ids"]), a["hcap"], a["id_stride"], a["label_at"], a["n"], a["T"], a["thr"],
                                     a["flags"], a["acap"], a["bcap"], p(a["sizes"]), p(a["gt_tab"]), p(a["hyp_tab"]), p(a["overlap"]))
    torch.cuda.synchronize()
    return rc, o


def raw_assign(ctx, weights, counts, fill=-7, **over):
    """the C entry with every output pre-filled; `over` replaces arguments by name -> (return code, outputs)"""
    import mi355_dt
    w, dims = weights, counts
    n, rcap, ccap = w.shape
    o = dict(r2c=torch.full((n, rcap), fill, dtype=torch.int32, device=ctx.device),
             c2r=torch.full((n, ccap), fill, dtype=torch.int32, device=ctx.device),
             total=torch.full((n,), fill, dtype=torch.int64, device=ctx.device))
    a = dict(w=w, rcap=rcap, ccap=ccap, dims=dims, stride=int(dims.shape[1]), rows_at=0, cols_at=1, n=n)
    a.update(o)
    a.update(over)
    p = lambda x: mi355_dt._dptr(x) if x is None or torch.is_tensor(x) else x
    ctx._sync_stream()
    rc = ctx.lib.dt_assign_max(ctx.h, p(a["w"]), a["rcap"], a["ccap"], p(a["dims"]), a["stride"], a["rows_at"], a["cols_at"], a["n"],
                               p(a["r2c"]), p(a["c2r"]), p(a["total"]))
    torch.cuda.synchronize()
    return rc, o


def untouched(o, fill=-7):
    return all(bool((v == fill).all()) for v in o.values())


# ------------------------------------------------------------------ 1. parity with the restatement
@pytest.mark.parametrize("any_label", [False, True])
@pytest.mark.parametrize("name", sorted(tsr.SCENES))
def test_parity_with_restatement(name, any_label):
    s, acap, bcap = isr.scene(name)
    ref = isr.scene_ref(name, any_label)
    idtp, idfn, idfp = isr.counts(ref)
    assert idtp > 0 and idfn > 0 and idfp > 0 and isr.splits(ref) > 0, "vacuous scene"
    same(gpu_score(ctx_(), s, any_label, acap, bcap), ref, "%s, any_label %s" % (name, any_label))


# ------------------------------------------------------------------ 2. both worked examples
def test_worked_examples():
    ctx = ctx_()
    got = gpu_score(ctx, tsr.worked_example(), False, 4, 4)
    assert got["sizes"].tolist() == isr.WORKED_SIZES
    assert got["gt_tab"].tolist() == isr.WORKED_GT_TAB + [[-1, 0]] * 3 and got["hyp_tab"].tolist() == isr.WORKED_HYP_TAB + [[-1, 0]] * 2
    assert got["overlap"][:1, :2].tolist() == isr.WORKED_OVERLAP and int(got["overlap"].sum()) == 5
    assert isr.counts(got) == (isr.WORKED_IDTP, isr.WORKED_IDFN, isr.WORKED_IDFP)
    assert got["gt_to_hyp"].tolist() == [1, -1, -1, -1] and got["hyp_to_gt"].tolist() == [-1, 0, -1, -1]
    same(got, isr.identity_score(thr=0.5, acap=4, bcap=4, **tsr.worked_example()), "worked example")
    (r2c, c2r, total), = gpu_assign(ctx, [np.array(isr.ANTI_GREEDY)])
    assert total == 8 and r2c.tolist() == [1, 0] and c2r.tolist() == [1, 0]


# ------------------------------------------------------------------ 3. a scene that crosses the 64-lane passes on every axis
def test_wide_scene():
    s, acap, bcap = isr.scene("ident_wide")
    ref = isr.scene_ref("ident_wide", False)
    assert s["gt_boxes"].shape[0] == 12 and s["gt_boxes"].shape[1] > 64 and ref["sizes"][3] > 64 and ref["sizes"][4] > 128
    assert (s["gt_counts"] > 64).any() and isr.counts(ref)[0] > 0 and isr.splits(ref) > 0
    same(gpu_score(ctx_(), s, False, acap, bcap), ref, "wide scene")


# ------------------------------------------------------------------ 4. full tables; ids < 0 and an id repeated within a frame
def test_table_overflow_on_each_side():
    ctx = ctx_()
    s, acap, bcap = isr.scene("small")
    full = isr.scene_ref("small", False)
    for ac, bc in ((4, bcap), (acap, 5), (4, 5)):
        ref = isr.scene_ref("small", False, acap=ac, bcap=bc)
        assert (ref["sizes"][5] > 0) == (ac == 4) and (ref["sizes"][6] > 0) == (bc == 5)
        assert ref["sizes"][3] == min(ac, full["sizes"][3]) and ref["sizes"][4] == min(bc, full["sizes"][4])
        same(gpu_score(ctx, s, False, ac, bc), ref, "acap %d, bcap %d" % (ac, bc))


def test_ids_below_zero_and_repeated_ids():
    """the parity scene `repeated_ids` has, in every frame, ground-truth rows of id -1 and ids shared by rows on both sides; and by hand:
    one frame, gt id 9 twice and id -1 once on one box, hypothesis id 5 twice on that box"""
    s, _, _ = isr.scene("repeated_ids")
    assert (s["gt_ids"][0, :int(s["gt_counts"][0])] < 0).any()
    assert len(set(s["gt_ids"][0, :int(s["gt_counts"][0])].tolist())) < int(s["gt_counts"][0]) - 1
    box = [0.4, 0.5, 0.2, 0.2, 1, 0, 1, 0]
    h = dict(gt_boxes=np.array([[box, box, box]], dtype=np.float32), gt_counts=np.array([3], dtype=np.int32),
             gt_ids=np.array([[9, -1, 9]], dtype=np.int32), hyp_boxes=np.array([[box, box, box]], dtype=np.float32),
             hyp_counts=np.array([3], dtype=np.int32), hyp_ids=np.array([[5, 5, -4]], dtype=np.int32))
    got = gpu_score(ctx_(), h, False, 2, 2)
    assert got["sizes"].tolist() == [1, 3, 3, 1, 1, 0, 0, 4] and got["gt_tab"].tolist() == [[9, 2], [-1, 0]]
    assert got["hyp_tab"].tolist() == [[5, 2], [-1, 0]] and got["overlap"].tolist() == [[4, 0], [0, 0]] and int(got["idtp"]) == 4
    same(got, isr.identity_score(*[h[k] for k in isr.INPUTS], thr=0.5, acap=2, bcap=2), "by hand")


# ------------------------------------------------------------------ 5. the solver alone
def assign_cases():
    if "assign" not in _REF:
        rs = np.random.RandomState(21)
        sparse = (rs.randint(1, 40, size=(200, 200)) * (rs.rand(200, 200) < 0.03)).astype(np.int64)
        mats = dict(one=np.array([[3]]), no_rows=np.zeros((0, 4), dtype=np.int64), anti_greedy=np.array(isr.ANTI_GREEDY),
                    wide=rs.randint(0, 50, size=(65, 130)), sparse=sparse)
        mats["tall"] = mats["wide"].T.copy()
        _REF["assign"] = mats
    return _REF["assign"]


@pytest.mark.parametrize("name", ["one", "no_rows", "anti_greedy", "wide", "tall", "sparse"])
def test_assign_max_shapes(name):
    m = assign_cases()[name]
    rcap, ccap = max(m.shape[0], 1) + 3, m.shape[1] + 2
    key = ("assign_ref", name)
    if key not in _REF:
        _REF[key] = ref_assign(m, rcap, ccap)
    r2c, c2r, total = _REF[key]
    isr.check_assignment(np.pad(m, ((0, rcap - m.shape[0]), (0, ccap - m.shape[1]))), m.shape[0], m.shape[1], r2c, c2r, total)
    ctx = ctx_()
    one, two = (gpu_assign(ctx, [m], rcap, ccap)[0] for _ in range(2))
    assert np.array_equal(one[0], r2c) and np.array_equal(one[1], c2r) and one[2] == total, name
    assert (one[0][m.shape[0]:] == -1).all() and (one[1][m.shape[1]:] == -1).all(), "rows and columns beyond the counts"
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and one[2] == two[2], "two runs, identical bits"
    if name == "tall":
        wide = gpu_assign(ctx, [assign_cases()["wide"]])[0]
        assert wide[2] == total, "the transpose has the same optimum"
    if name == "sparse":
        assert (r2c[:200] < 0).any() and total > 0, "vacuous: a sparse matrix leaves rows unassigned"


def test_assign_max_batch_of_48_and_dims_with_a_stride():
    rs = np.random.RandomState(33)
    if "batch" not in _REF:
        mats = [rs.randint(0, 6 if k % 3 else 100, size=(rs.randint(0, 25), rs.randint(0, 41))) for k in range(48)]
        _REF["batch"] = (mats, [ref_assign(m, 24, 40) for m in mats])
    mats, refs = _REF["batch"]
    assert len({m.shape for m in mats}) > 40 and any(m.shape[0] > m.shape[1] for m in mats)
    for stride in (None, 8):
        got = gpu_assign(ctx_(), mats, 24, 40, dims_stride=stride)
        for k in range(48):
            assert np.array_equal(got[k][0], refs[k][0]) and np.array_equal(got[k][1], refs[k][1]) and got[k][2] == refs[k][2], (stride, k)
    # dims = None: every problem is rcap x ccap
    ctx = ctx_()
    w = rs.randint(0, 9, size=(3, 5, 4)).astype(np.int32)
    r2c, c2r, total = ctx.assign_max(dev(w, ctx))
    for k in range(3):
        ref = isr.assign_max(w[k])
        assert np.array_equal(r2c[k].cpu().numpy(), ref[0]) and np.array_equal(c2r[k].cpu().numpy(), ref[1]) and int(total[k]) == ref[2]


# ------------------------------------------------------------------ 6. the chunk contract
def test_chunks_equal_one_call():
    ctx = ctx_()
    if "chunk" not in _REF:
        s = tsr.make_scene(30, 32, 32, 12, 7, duplicates=True)
        bcap = len(isr.hyp_ids_of(s)) + 3
        _REF["chunk"] = (s, bcap, isr.identity_score(*[s[k] for k in isr.INPUTS], thr=0.5, acap=64, bcap=bcap))
    s, bcap, ref = _REF["chunk"]
    assert s["gt_boxes"].shape[0] == 30
    whole = gpu_score(ctx, s, False, 64, bcap)
    same(whole, ref, "one call")
    same(gpu_score(ctx, s, False, 64, bcap, chunks=[1, 7, 22]), whole, "chunks (1, 7, 22)")
    dropped = gpu_score(ctx, s, False, 64, bcap, chunks=[1, 7, 22], resume=False)
    assert not np.array_equal(dropped["sizes"], whole["sizes"]) and not np.array_equal(dropped["overlap"], whole["overlap"]), \
        "vacuous: the last chunk does not depend on the state"


# ------------------------------------------------------------------ 7. uninitialised output buffers
def test_uninitialised_outputs_are_fully_written():
    ctx = ctx_()
    s, acap, bcap = isr.scene("small")
    ref = isr.scene_ref("small", False)
    rc, o = raw_overlap(ctx, on_dev(ctx, s), acap, bcap)
    assert rc == 0
    same(to_host(o, keys=isr.KEYS), ref, "overlap buffers pre-filled with -7", isr.KEYS)
    w = np.zeros((2, 5, 9), dtype=np.int32)
    w[0, :2, :2] = isr.ANTI_GREEDY
    rc, a = raw_assign(ctx, dev(w, ctx), dev(np.array([[2, 2], [0, 0]], dtype=np.int32), ctx))
    assert rc == 0 and a["total"].tolist() == [8, 0]
    assert a["r2c"].tolist() == [[1, 0, -1, -1, -1], [-1] * 5] and a["c2r"].tolist() == [[1, 0] + [-1] * 7, [-1] * 9]


# ------------------------------------------------------------------ 8. errors
def test_errors_leave_the_outputs_untouched():
    ctx = ctx_()
    s, acap, bcap = isr.scene("small")
    ref = isr.scene_ref("small", False)
    d = on_dev(ctx, s)
    gcap, hcap = d[0].shape[2], d[3].shape[2]
    words = lambda ac: 2 * ac + 2 * bcap + 7 * gcap + 7 * hcap
    fits = (40960 - 2 * bcap - 7 * gcap - 7 * hcap) // 2
    assert words(fits) <= 40960 < words(fits + 1)
    bad = [dict(gt_boxes=None), dict(gt_counts=None), dict(gt_ids=None), dict(hyp_boxes=None), dict(hyp_counts=None), dict(hyp_ids=None),
           dict(sizes=None), dict(gt_tab=None), dict(hyp_tab=None), dict(overlap=None),
           dict(n=-1), dict(T=0), dict(T=-3), dict(gcap=0), dict(hcap=0), dict(hcap=-1), dict(acap=0), dict(acap=-2), dict(bcap=0),
           dict(bcap=-1), dict(id_stride=0), dict(label_at=-1), dict(label_at=8), dict(flags=4), dict(flags=8 | ANY), dict(flags=-1),
           dict(thr=float("nan")), dict(thr=0.0), dict(thr=-0.1), dict(thr=1.5), dict(thr=float("inf")), dict(acap=fits + 1),
           dict(n=1 << 19, acap=64, bcap=64)]
    for over in bad:                     # (the buffers keep the scene's sizes; only the arguments change)
        rc, o = raw_overlap(ctx, d, acap, bcap, **over)
        assert rc == ARG and untouched(o), over
    rc, o = raw_overlap(ctx, d, acap, bcap, n=0)
    assert rc == 0 and untouched(o), "n_clips = 0 is a no-op"
    with pytest.raises(Exception):
        ctx.identity_overlap(*d, iou_threshold=0.0, gt_cap=acap, hyp_cap=bcap)
    # the solver's
    w = dev(np.ones((2, 4, 6), dtype=np.int32), ctx)
    dims = dev(np.array([[4, 6, 0], [4, 6, 0]], dtype=np.int32), ctx)
    bad = [dict(w=None), dict(dims=None), dict(r2c=None), dict(c2r=None), dict(total=None), dict(n=-1), dict(rcap=0), dict(rcap=-1),
           dict(ccap=0), dict(rows_at=-1), dict(rows_at=3), dict(cols_at=3), dict(cols_at=-2), dict(stride=0), dict(stride=1),
           dict(n=1 << 27), dict(rcap=6825 + 1), dict(ccap=1 << 16)]
    for over in bad:
        rc, o = raw_assign(ctx, w, dims, **over)
        assert rc == ARG and untouched(o), over
    rc, o = raw_assign(ctx, w, dims, n=0)
    assert rc == 0 and untouched(o), "n = 0 is a no-op"
    # following valid calls are unaffected -- and the largest table that fits the LDS launches
    rc, o = raw_assign(ctx, w, dims)
    assert rc == 0 and o["total"].tolist() == [4, 4]
    rc, o = raw_overlap(ctx, d, acap, bcap)
    assert rc == 0
    same(to_host(o, keys=isr.KEYS), ref, "after the refused calls", isr.KEYS)
    rc, o = raw_overlap(ctx, d, fits, bcap, thr=1.0)
    assert rc == 0
    got = to_host(o, keys=isr.KEYS)
    assert np.array_equal(got["gt_tab"][:acap], ref["gt_tab"]) and (got["gt_tab"][acap:] == [-1, 0]).all()
    assert got["sizes"][1] == ref["sizes"][1] and got["sizes"][7] < ref["sizes"][7], "threshold 1 keeps fewer pairs"


# ------------------------------------------------------------------ 9. the tracker's own method, on its own result
def test_tracker_identity_on_a_track_clips_result():
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
        plain = trk.identity(res, gt)
        ctx.profile_enable(False)
        assert "associate:identity_overlap" in ctx.profile_names() and "associate:assign_max" in ctx.profile_names()
        p = evaluate.identity(plain)["pooled"]
        assert (p["gt"], p["hyp"], p["idtp"], p["idfn"], p["idfp"], p["overflow"]) == (total, total, total, 0, 0, 0)
        assert p["idf1"] == 1.0 and p["gt_tracks"] == p["hyp_tracks"] == int(res["nids"].sum())
        # the confirmed-track read-out of the same boxes as hypotheses
        with pytest.raises(Exception):
            trk.identity(res, gt, confirmed=True)
        a = ctx.associate_tracks(res["boxes"], res["counts"], trk.ASSOC_THRESHOLD, 2, 0.5, 2, track_cap=cap)
        conf = trk.identity(dict(res, tracks=a["tracks"], track_counts=a["track_counts"], track_info=a["track_info"]), gt, confirmed=True)
        for k in range(n):
            ref = isr.identity_score(*[x[k].cpu().numpy() for x in gt], a["tracks"][k].cpu().numpy(), a["track_counts"][k].cpu().numpy(),
                                     a["track_info"][k].cpu().numpy(), thr=0.5, acap=int(conf["gt_tab"].shape[1]),
                                     bcap=int(conf["hyp_tab"].shape[1]), label_at=4)
            same(to_host(conf, k), ref, "confirmed, clip %d" % k)
        q = evaluate.identity(conf)["pooled"]
        assert q["hyp"] != p["hyp"] and 0 < q["idtp"] < total, "vacuous: the read-out scores as the boxes do"


# ------------------------------------------------------------------ 10. many clips in one call
def test_48_clips_in_one_call():
    ctx = ctx_()
    T, cap, acap, bcap = 30, 16, 32, 96
    if "clips48" not in _REF:
        scenes = [tsr.make_scene(T, cap, cap, 6 + k % 5, 100 + k) for k in range(48)]
        refs = [isr.identity_score(*[s[k] for k in isr.INPUTS], thr=0.5, acap=acap, bcap=bcap) for s in scenes]
        _REF["clips48"] = (scenes, refs)
    scenes, refs = _REF["clips48"]
    d = [dev(np.stack([s[k] for s in scenes]), ctx) for k in isr.INPUTS]
    got = ctx.identity_score(*d, gt_cap=acap, hyp_cap=bcap)
    for k in range(48):
        same(to_host(got, k), refs[k], "clip %d" % k)
    assert len(set(tuple(r["sizes"]) for r in refs)) > 40, "the clips must differ"
    assert all(r["sizes"][6] == 0 for r in refs)


# ------------------------------------------------------------------ 11. the library exports the entries
def test_library_exports_the_entries():
    import mi355_dt
    out = subprocess.run(["nm", "-D", "--defined-only", mi355_dt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("dt_identity_overlap", "dt_assign_max"):
        assert name in exported and name in mi355_dt.SYMBOLS
    assert mi355_dt.DT_IDENT_INTS == 8
    assert ctx_().lib.dt_abi_version() == 108
