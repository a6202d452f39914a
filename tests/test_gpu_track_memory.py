"""GPU suite (-m gpu): track memory -- a lost track keeps its id for up to max_age frames.

Ids and gaps are integers and decode.hip forms no fused multiply-add, so everything here is array_equal / torch.equal against
the plain restatement tests/track_memory_ref.py (whose IoU is the oracle's), and at max_age = 0 against orc.associate_clip and
the entries that existed before.  Both kernel forms are covered: registers (tcap <= 64 and T <= 64) and LDS (any tcap).
"""
import re

import numpy as np
import pytest
import torch

from oracle import oracle as orc

from utility import synth

import track_memory_ref as tm

pytestmark = pytest.mark.gpu

THR = 0.3
AGES = (1, 3, 8)

_CACHE = {}


def dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def small_tracker():
    """96x128 (3x4 grid), C = 12: a context for the association entries, and a model whose reload makes every slot fresh"""
    if "small" not in _CACHE:
        from models_tracking.MultiObjDetTracker import MultiObjDetTracker

        class Trk(MultiObjDetTracker):
            IMAGE_H, IMAGE_W = 96, 128
            GRID_H, GRID_W = 3, 4
            SEQUENCE_LENGTH = 4
            LOAD_MODEL = False
            OBJ_THRESHOLD = 0.3

        C = len(Trk.LABELS)
        blob = synth.synth_darknet_blob(C)
        tw = synth.synth_tracker_weights(C)
        _CACHE["small"] = (Trk(detector_weights=blob, tracker_weights=tw), blob, tw)
    return _CACHE["small"]


def big_tracker():
    """416x416, calibrated by bench.build_tracker to ~32 boxes per frame, and 2 x 30 frames of bench.make_frames
    (the construction of tests/test_gpu_stream.py)"""
    if "big" not in _CACHE:
        import bench
        d = torch.device("cuda", torch.cuda.current_device())
        frames = bench.make_frames(2, 30, 416, 416, d, seed0=42)
        trk, blob, tw = bench.build_tracker(416, 416, 30, 32, frames[:1])
        _CACHE["big"] = (trk, blob, tw, frames)
    return _CACHE["big"]


def ctx_():
    return small_tracker()[0].model.ctx


def gpu_clip(ctx, boxes, counts, max_age, tcap):
    ids, nids, gaps = ctx.associate(dev(boxes[None], ctx), dev(counts[None], ctx), THR, max_age=max_age, track_cap=tcap, want_gaps=True)
    return ids[0].cpu().numpy(), int(nids[0]), gaps[0].cpu().numpy()


def gpu_chunked(ctx, boxes, counts, chunks, slot, max_age, old_entry_at=()):
    """one stream through slot `slot`; max_age an int or one per CHUNK; chunks whose index is in old_entry_at go through
    dt_associate_stream, which has no gaps to give (None in the returned list of per-chunk gaps)"""
    ids, gaps, nid, t0 = [], [], None, 0
    for k, L in enumerate(chunks):
        b, c = dev(boxes[None, t0:t0 + L], ctx), dev(counts[None, t0:t0 + L], ctx)
        if k in old_entry_at:
            i, nid = ctx.associate_stream(b, c, THR, [slot])
            g = None
        else:
            a = max_age if np.isscalar(max_age) else max_age[k]
            i, nid, g = ctx.associate_stream(b, c, THR, [slot], max_age=a, want_gaps=True)
        ids.append(i[0].cpu().numpy())
        gaps.append(g[0].cpu().numpy() if g is not None else None)
        t0 += L
    assert t0 == boxes.shape[0]
    return np.concatenate(ids), int(nid[0]), gaps


def check(got, ref, what):
    ids, nids, gaps = got
    rid, rn, rg = ref[:3]
    bad = np.nonzero((ids != rid).any(1))[0]
    assert bad.size == 0, "%s: ids differ from the restatement at frames %s" % (what, bad[:8])
    bad = np.nonzero((gaps != rg).any(1))[0]
    assert bad.size == 0, "%s: gaps differ from the restatement at frames %s" % (what, bad[:8])
    assert nids == rn, "%s: %d ids opened, restatement %d" % (what, nids, rn)


# ------------------------------------------------------------------ 1 + 2. parity with the restatement, not vacuous
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_parity_with_restatement(case):
    T, cap, n_obj_t, tcap, _ = tm.CASES[case]
    ctx = ctx_()
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    if "register" in case or case == "empty_frames":
        assert tcap <= 64 and T <= 64      # the register form
    if "over_64" in case:
        assert counts.max() > 64 and counts.min() <= 64
    refs = {a: tm.associate_memory(boxes, counts, THR, a, tcap) for a in (0,) + AGES}
    assert refs[3][1] < refs[0][1], "vacuous: memory bridges nothing (%d ids with max_age 3, %d without)" % (refs[3][1], refs[0][1])
    assert (refs[3][2] >= 2).any(), "vacuous: no track re-acquired after two missed frames"
    print("%s: ids opened %s, boxes with gap >= 2 at max_age 3: %d, entries cut by tcap %s" % (
        case, {a: r[1] for a, r in refs.items()}, int((refs[3][2] >= 2).sum()), {a: r[3] for a, r in refs.items()}))
    for a in AGES:
        check(gpu_clip(ctx, boxes, counts, a, tcap), refs[a], "%s, max_age %d" % (case, a))


def test_figures_of_the_sizing_cases():
    n = {}
    for case in ("register_form", "register_form_edge", "lds_form"):
        T, cap, n_obj_t, tcap, _ = tm.CASES[case]
        boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
        r0, r3 = (tm.associate_memory(boxes, counts, THR, a, tcap) for a in (0, 3))
        n[case] = (r0[1], r3[1])
        if case == "register_form":
            assert int((r3[2] > 0).sum()) == 64
        check(gpu_clip(ctx_(), boxes, counts, 3, tcap), r3, case)
    assert n == {"register_form": (119, 55), "register_form_edge": (259, 152), "lds_form": (290, 214)}


def test_many_clips_in_one_call():
    """one wavefront per clip: clips of both kinds of content in one launch, and d_gaps == NULL"""
    ctx = ctx_()
    T, cap, tcap = 12, 128, 160
    seqs = [tm.moving_boxes(T, cap, (lambda t, k=k: 10 + 30 * k), seed=40 + k) for k in range(5)]
    b = np.stack([s[0] for s in seqs]); c = np.stack([s[1] for s in seqs])
    ids, nids, gaps = ctx.associate(dev(b, ctx), dev(c, ctx), THR, max_age=3, track_cap=tcap, want_gaps=True)
    ids2, nids2 = ctx.associate(dev(b, ctx), dev(c, ctx), THR, max_age=3, track_cap=tcap)
    assert torch.equal(ids, ids2) and torch.equal(nids, nids2)
    for k in range(5):
        check((ids[k].cpu().numpy(), int(nids[k]), gaps[k].cpu().numpy()), tm.associate_memory(seqs[k][0], seqs[k][1], THR, 3, tcap), "clip %d" % k)


# ------------------------------------------------------------------ 3. the capacity cut
@pytest.mark.parametrize("form", ["lds", "registers"])
def test_capacity_cut(form):
    """lds: 120 then 20 objects, tcap 160, max_age 8 (41 entries cut).  registers: 30 objects in frames of at most 32 boxes with
    a table of 40 entries -- the cut inside the register form's lane permutation."""
    ctx = ctx_()
    if form == "lds":
        T, cap, n_obj_t, tcap, _ = tm.CASES["table_over_64_then_small"]
        roomy = 256
    else:
        T, cap, n_obj_t, tcap, roomy = 40, 32, (lambda t: 30), 40, 64
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    tight = tm.associate_memory(boxes, counts, THR, 8, tcap)
    loose = tm.associate_memory(boxes, counts, THR, 8, roomy)
    print("%s: tcap %d cuts %d entries, tcap %d cuts %d; ids differ in %d places" % (form, tcap, tight[3], roomy, loose[3], int((tight[0] != loose[0]).sum())))
    assert tight[3] > 0 and loose[3] == 0
    if form == "lds":
        assert tight[3] == 41
    assert (tight[0] != loose[0]).any(), "the cut changes no id: the test would not see it"
    got_t, got_l = gpu_clip(ctx, boxes, counts, 8, tcap), gpu_clip(ctx, boxes, counts, 8, roomy)
    check(got_t, tight, "tcap %d" % tcap)
    check(got_l, loose, "tcap %d" % roomy)
    assert (got_t[0] != got_l[0]).any()


# ------------------------------------------------------------------ 4. max_age = 0 through the new entries
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_max_age_0_equals_the_present_entries(case):
    T, cap, n_obj_t, tcap, chunkings = tm.CASES[case]
    ctx = ctx_()
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    rid, rn = orc.associate_clip(boxes, counts, THR)
    b, c = dev(boxes[None], ctx), dev(counts[None], ctx)
    old_ids, old_n = ctx.associate(b, c, THR)
    for tc in sorted({cap, tcap}):
        ids, nids, gaps = ctx.associate(b, c, THR, max_age=0, track_cap=tc, want_gaps=True)
        assert torch.equal(ids, old_ids) and torch.equal(nids, old_n), "tcap %d" % tc
        assert np.array_equal(ids[0].cpu().numpy(), rid) and int(nids[0]) == rn
        g = gaps[0].cpu().numpy()
        assert set(np.unique(g)) <= {-1, 0}
        assert np.array_equal(g, tm.associate_memory(boxes, counts, THR, 0, tc)[2])
    ctx.stream_open(3, cap, track_cap=tcap)
    for chunks in chunkings:
        ctx.stream_reset([1, 2])
        ids, nid, gaps = gpu_chunked(ctx, boxes, counts, chunks, 1, 0)
        old, old_nid, _ = gpu_chunked(ctx, boxes, counts, chunks, 2, 0, old_entry_at=range(len(chunks)))
        assert np.array_equal(ids, rid) and nid == rn, "chunks %s" % chunks
        assert np.array_equal(old, rid) and old_nid == rn, "dt_associate_stream on a table of %d entries, chunks %s" % (tcap, chunks)
        assert set(np.unique(np.concatenate(gaps))) <= {-1, 0}


# ------------------------------------------------------------------ 5. chunk invariance for streams
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_stream_chunk_invariance(case):
    T, cap, n_obj_t, tcap, chunkings = tm.CASES[case]
    ctx = ctx_()
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    ctx.stream_open(2, cap, track_cap=tcap)
    for a in AGES:
        ref = tm.associate_memory(boxes, counts, THR, a, tcap)
        whole = gpu_clip(ctx, boxes, counts, a, tcap)
        check(whole, ref, "%s stateless" % case)
        for chunks in chunkings:
            ctx.stream_reset([1])
            ids, nid, gaps = gpu_chunked(ctx, boxes, counts, chunks, 1, a)
            check((ids, nid, np.concatenate(gaps)), ref, "%s, max_age %d, chunks %s" % (case, a, chunks))


def test_5_streams_out_of_step():
    """the schedule of test_associate_stream_5_streams_out_of_step with max_age = 3: 10 .. 82 objects, so one call carries
    tables below and above 64 live entries; tcap 128 > cap 96"""
    ctx = ctx_()
    n, T, cap, tcap = 5, 40, 96, 128
    seqs = [tm.moving_boxes(T, cap, (lambda t, k=k: 10 + 18 * k), seed=20 + k) for k in range(n)]
    refs = [tm.associate_memory(b, c, THR, 3, tcap) for b, c in seqs]
    slot = [6, 0, 3, 8, 1]
    ctx.stream_open(9, cap, track_cap=tcap)
    cur, got, gg, nid, call = [0] * n, [[] for _ in range(n)], [[] for _ in range(n)], [0] * n, 0
    lengths = [3, 1, 7, 2, 5, 4]
    cuts = [[] for _ in range(n)]
    while min(cur) < T:
        L = lengths[call % len(lengths)]
        who = [k for k in range(n) if call % (k + 2) != 0 and cur[k] + L <= T]
        if not who:
            L, who = 1, [k for k in range(n) if cur[k] < T]
        who = who[call % len(who):] + who[:call % len(who)]
        b = np.stack([seqs[k][0][cur[k]:cur[k] + L] for k in who])
        c = np.stack([seqs[k][1][cur[k]:cur[k] + L] for k in who])
        ids, nids, gaps = ctx.associate_stream(dev(b, ctx), dev(c, ctx), THR, [slot[k] for k in who], max_age=3, want_gaps=True)
        for j, k in enumerate(who):
            got[k].append(ids[j].cpu().numpy()); gg[k].append(gaps[j].cpu().numpy()); nid[k] = int(nids[j]); cur[k] += L; cuts[k].append(L)
        call += 1
    assert len({tuple(c) for c in cuts}) == n
    for k in range(n):
        assert (refs[k][2] >= 2).any()
        check((np.concatenate(got[k]), nid[k], np.concatenate(gg[k])), refs[k], "stream %d (chunks %s)" % (k, cuts[k]))


# ------------------------------------------------------------------ 6. mixed calls on one slot
@pytest.mark.parametrize("case", ["register_form", "table_over_64_then_small"])
def test_mixed_max_age_on_one_slot(case):
    T, cap, n_obj_t, tcap, _ = tm.CASES[case]
    ctx = ctx_()
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    third = T // 3
    chunks, ages = [third, third, T - 2 * third], [3, 0, 3]
    per_frame = sum(([a] * L for a, L in zip(ages, chunks)), [])
    ref = tm.associate_memory(boxes, counts, THR, per_frame, tcap)
    assert ref[1] not in (tm.associate_memory(boxes, counts, THR, 3, tcap)[1], tm.associate_memory(boxes, counts, THR, 0, tcap)[1])
    ctx.stream_open(2, cap, track_cap=tcap)
    ids, nid, gaps = gpu_chunked(ctx, boxes, counts, chunks, 0, ages)
    check((ids, nid, np.concatenate(gaps)), ref, "max_age 3, 0, 3")
    # the middle chunk through dt_associate_stream: the same ids (that entry has no gaps to give)
    ids2, nid2, gaps2 = gpu_chunked(ctx, boxes, counts, chunks, 1, ages, old_entry_at=(1,))
    assert np.array_equal(ids2, ref[0]) and nid2 == ref[1]
    assert np.array_equal(gaps2[0], ref[2][:third]) and np.array_equal(gaps2[2], ref[2][2 * third:])


@pytest.mark.parametrize("case", ["register_form", "table_small_then_over_64"])
def test_old_and_new_entry_interleaved_at_max_age_0(case):
    T, cap, n_obj_t, tcap, _ = tm.CASES[case]
    ctx = ctx_()
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    ref = tm.associate_memory(boxes, counts, THR, 0, tcap)
    rid, rn = orc.associate_clip(boxes, counts, THR)
    assert np.array_equal(ref[0], rid) and ref[1] == rn
    chunks = [1, 2] * (T // 3) + [1] * (T % 3)
    ctx.stream_open(1, cap, track_cap=tcap)
    ids, nid, _ = gpu_chunked(ctx, boxes, counts, chunks, 0, 0, old_entry_at=range(0, len(chunks), 2))
    assert np.array_equal(ids, rid) and nid == rn


# ------------------------------------------------------------------ 7. slots independent, reset and reload
def test_slots_independent_reset_and_reload():
    trk, _, tw = small_tracker()
    ctx = trk.model.ctx
    T, cap, tcap = 24, 32, 64
    A = tm.moving_boxes(T, cap, lambda t: 12, seed=7)
    B = tm.moving_boxes(T, cap, lambda t: 14, seed=8)
    refA, refB = (tm.associate_memory(b, c, THR, 3, tcap) for b, c in (A, B))
    refA_head = tm.associate_memory(A[0][:12], A[1][:12], THR, 3, tcap)
    ctx.stream_open(4, cap, track_cap=tcap)

    def call(parts, slots):
        b = np.stack([p[0] for p in parts]); c = np.stack([p[1] for p in parts])
        ids, nids, gaps = ctx.associate_stream(dev(b, ctx), dev(c, ctx), THR, slots, max_age=3, want_gaps=True)
        return ids.cpu().numpy(), nids.cpu().numpy(), gaps.cpu().numpy()

    cut = lambda s, a, b: (s[0][a:b], s[1][a:b])
    i1, n1, g1 = call([cut(A, 0, 12), cut(B, 0, 12)], [3, 1])
    ctx.stream_reset([3])
    # slot 3 starts over on A's first half (ids from 0, an empty table); slot 1 goes on with B, aged entries and all
    i2, n2, g2 = call([cut(B, 12, 24), cut(A, 0, 12)], [1, 3])
    assert np.array_equal(i2[1], refA_head[0]) and n2[1] == refA_head[1] and np.array_equal(g2[1], refA_head[2])
    assert np.array_equal(i1[0], refA_head[0])
    check((np.concatenate([i1[1], i2[0]]), int(n2[0]), np.concatenate([g1[1], g2[0]])), refB, "neighbour of a reset slot")
    assert (refB[2][12] > 0).any() or (refB[2][12:14] > 0).any(), "vacuous: no aged entry of slot 1 was claimed right after the reset"
    # slot 3 goes on: the whole of A
    i3, n3, g3 = call([cut(A, 12, 24)], [3])
    check((np.concatenate([i2[1], i3[0]]), int(n3[0]), np.concatenate([g2[1], g3[0]])), refA, "the reset slot, continued")
    # a load makes every slot fresh
    trk.model.set_weights(tw)
    i4, n4, g4 = call([cut(A, 0, 12), cut(B, 0, 12)], [3, 1])
    assert np.array_equal(i4, i1) and np.array_equal(n4, n1) and np.array_equal(g4, g1)


# ------------------------------------------------------------------ 8. errors
def _code(excinfo):
    return int(re.search(r"failed \((\d+)\)", str(excinfo.value)).group(1))


def test_errors_leave_the_state_unchanged():
    import mi355_dt
    trk, blob, tw = small_tracker()
    ctx = trk.model.ctx
    ARG, STATE = 1, 3
    T, cap, tcap = 20, 32, 64
    boxes, counts = tm.moving_boxes(T, cap, lambda t: 12, seed=7)
    ref = tm.associate_memory(boxes, counts, THR, 3, tcap)
    b = lambda a, z: dev(boxes[None, a:z], ctx)
    c = lambda a, z: dev(counts[None, a:z], ctx)

    fresh = type(trk)(detector_weights=blob, tracker_weights=tw)      # no stream_open yet
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.model.ctx.associate_stream(b(0, 4), c(0, 4), THR, [0], max_age=3)
    assert _code(e) == STATE
    fresh.model.ctx.close()

    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.stream_open(4, cap, track_cap=cap - 1)
    assert _code(e) == ARG
    for bad_age, bad_cap in ((-1, 64), (3, 31)):
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate(b(0, 4), c(0, 4), THR, max_age=bad_age, track_cap=bad_cap)
        assert _code(e) == ARG
    with pytest.raises(mi355_dt.NativeError) as e:      # a table beyond the LDS: refused, never launched
        ctx.associate(b(0, 4), c(0, 4), THR, max_age=3, track_cap=4096)
    assert _code(e) == ARG

    ctx.stream_open(4, cap, track_cap=tcap)
    i1, n1, g1 = ctx.associate_stream(b(0, 9), c(0, 9), THR, [2], max_age=3, want_gaps=True)
    for bad in ([4], [-1]):
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_stream(b(9, 20), c(9, 20), THR, bad, max_age=3)
        assert _code(e) == ARG, bad
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_stream(dev(boxes[None, 9:11].repeat(2, 0), ctx), dev(counts[None, 9:11].repeat(2, 0), ctx), THR, [2, 2], max_age=3)
    assert _code(e) == ARG
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_stream(b(9, 20), c(9, 20), THR, [2], max_age=-1)
    assert _code(e) == ARG
    with pytest.raises(mi355_dt.NativeError) as e:      # cap differs from the table's
        ctx.associate_stream(dev(boxes[None, 9:20, :31], ctx), c(9, 20), THR, [2], max_age=3)
    assert _code(e) == ARG
    n, arr = ctx._slot_array([2])
    assert ctx.lib.dt_associate_stream_mem(ctx.h, None, None, 1, 3, cap, 0.3, 3, arr, None, None, None) == ARG
    i2, n2, g2 = ctx.associate_stream(b(9, 20), c(9, 20), THR, [2], max_age=3, want_gaps=True)
    check((np.concatenate([i1[0].cpu().numpy(), i2[0].cpu().numpy()]), int(n2[0]),
           np.concatenate([g1[0].cpu().numpy(), g2[0].cpu().numpy()])), ref, "after the refused calls")
    assert (ref[2][9:] > 0).any(), "vacuous: the second chunk claims no aged entry"


# ------------------------------------------------------------------ 9. end to end at 416
def test_end_to_end_416_chunks_equal_clip():
    from parallel import pinned_policy
    trk, blob, tw, fr = big_tracker()

    class Mem(type(trk)):
        MAX_AGE = 3

    mem = Mem(detector_weights=blob, tracker_weights=tw)
    try:
        keys = ("netout", "boxes", "counts", "ids", "gaps")
        mem.open_streams(2)
        with pinned_policy(mem.model.ctx):
            ref = mem.track_clips(fr[:1])
            parts, t0 = [], 0
            for L in (12, 6, 12):
                parts.append(mem.track_stream(fr[:1, t0:t0 + L], [1]))
                t0 += L
        assert set(ref) == set(keys) | {"nids"}
        for k in keys:
            assert torch.equal(torch.cat([p[k] for p in parts], dim=1), ref[k]), k
        assert torch.equal(parts[-1]["nids"], ref["nids"])
        assert int(ref["counts"].sum()) > 0
        g = ref["gaps"]
        assert int(g.min()) >= -1 and int(g.max()) <= 3
        # the restatement on the boxes the GPU decoded
        b, c = ref["boxes"][0].cpu().numpy(), ref["counts"][0].cpu().numpy()
        r = tm.associate_memory(b, c, mem.ASSOC_THRESHOLD, 3, b.shape[1])
        check((ref["ids"][0].cpu().numpy(), int(ref["nids"][0]), g[0].cpu().numpy()), r, "416, one clip")
        bbs = mem.boxes_from_result(ref, 0)
        t_first = next(t for t in range(30) if c[t] > 0)
        assert bbs[t_first][0].track_gap == int(g[0, t_first, 0]) and bbs[t_first][0].track_id == int(ref["ids"][0, t_first, 0])
    finally:
        mem.model.ctx.close()


def test_max_age_0_result_is_todays():
    from parallel import pinned_policy
    trk, _, _, fr = big_tracker()
    assert trk.MAX_AGE == 0 and trk.TRACK_CAP is None
    trk.open_streams(1)
    ctx = trk.model.ctx
    with pinned_policy(ctx):
        ctx.profile_reset(); ctx.profile_enable(True)
        ref = trk.track_clips(fr[:1])
        got = trk.track_stream(fr[:1], [0])
        ctx.profile_enable(False)
    names = ctx.profile_names()
    assert "associate:memory" not in names and "associate:stream_memory" not in names, "MAX_AGE = 0 must keep today's launches"
    assert ctx.profile_read("associate")["launches"] == 2
    assert set(ref) == set(got) == {"boxes", "counts", "ids", "nids", "netout"}
    rid, rn = orc.associate_clip(ref["boxes"][0].cpu().numpy(), ref["counts"][0].cpu().numpy(), trk.ASSOC_THRESHOLD)
    for r in (ref, got):
        assert np.array_equal(r["ids"][0].cpu().numpy(), rid) and int(r["nids"][0]) == rn
    assert all(bb.track_gap is None for frame in trk.boxes_from_result(ref, 0) for bb in frame)
