"""GPU suite (-m gpu): track motion -- a track is matched where its constant velocity predicts it.

Ids and gaps are integers, decode.hip forms no fused multiply-add and its division is the correctly rounded one, so everything
here is array_equal / torch.equal against the plain restatement tests/track_motion_ref.py (whose IoU is the oracle's), and at
gain 0 against dt_associate_mem.  Both kernel forms are covered: registers (tcap <= 64 and T <= 64) and LDS (any tcap).
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import track_memory_ref as tm
import track_motion_ref as tmo

from test_gpu_track_memory import big_tracker, check, dev, small_tracker

pytestmark = pytest.mark.gpu

THR = 0.3
AGES = (0, 1, 3)
GAINS = (0.5, 1.0)

_REF = {}


def ctx_():
    return small_tracker()[0].model.ctx


def seq(case, seed=7):
    T, cap, n_obj_t, tcap, chunkings = tm.CASES[case]
    key = ("seq", case, seed)
    if key not in _REF:
        _REF[key] = tm.moving_boxes(T, cap, n_obj_t, seed=seed)
    return _REF[key] + (tcap, chunkings)


def ref_of(case, max_age, gain):
    """the restatement on a tm.CASES entry (seed 7), computed once for all the tests that want it"""
    key = (case, max_age, gain)
    if key not in _REF:
        boxes, counts, tcap, _ = seq(case)
        _REF[key] = tmo.associate_motion(boxes, counts, THR, max_age, gain, tcap)
    return _REF[key]


def gpu_clip(ctx, boxes, counts, max_age, gain, tcap):
    ids, nids, gaps = ctx.associate(dev(boxes[None], ctx), dev(counts[None], ctx), THR, max_age=max_age, track_cap=tcap, want_gaps=True,
                                    motion_gain=gain)
    return ids[0].cpu().numpy(), int(nids[0]), gaps[0].cpu().numpy()


def gpu_chunked(ctx, boxes, counts, chunks, slot, max_age, gain, mem_at=(), old_at=()):
    """one stream through slot `slot`; chunks whose index is in mem_at go through dt_associate_stream_mem, those in old_at
    through dt_associate_stream (which has no gaps to give: None in the returned list of per-chunk gaps)"""
    ids, gaps, nid, t0 = [], [], None, 0
    for k, L in enumerate(chunks):
        b, c = dev(boxes[None, t0:t0 + L], ctx), dev(counts[None, t0:t0 + L], ctx)
        if k in old_at:
            i, nid = ctx.associate_stream(b, c, THR, [slot])
            g = None
        elif k in mem_at:
            i, nid, g = ctx.associate_stream(b, c, THR, [slot], max_age=max_age, want_gaps=True)
        else:
            i, nid, g = ctx.associate_stream(b, c, THR, [slot], max_age=max_age, want_gaps=True, motion_gain=gain)
        ids.append(i[0].cpu().numpy())
        gaps.append(g[0].cpu().numpy() if g is not None else None)
        t0 += L
    assert t0 == boxes.shape[0]
    return np.concatenate(ids), int(nid[0]), gaps


# ------------------------------------------------------------------ 1. parity with the restatement
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_parity_with_restatement(case):
    boxes, counts, tcap, _ = seq(case)
    T = boxes.shape[0]
    ctx = ctx_()
    if "register" in case or case == "empty_frames":
        assert tcap <= 64 and T <= 64      # the register form
    if "over_64" in case:
        assert counts.max() > 64 and counts.min() <= 64
    mem3 = tm.associate_memory(boxes, counts, THR, 3, tcap)
    for g in GAINS:
        r3 = ref_of(case, 3, g)
        assert not np.array_equal(r3[0], mem3[0]), "vacuous: the velocities change no id (gain %g)" % g
        print("%s, gain %g: ids opened %s (memory rule at max_age 3: %d), entries cut by tcap %s" % (
            case, g, {a: ref_of(case, a, g)[1] for a in AGES}, mem3[1], {a: ref_of(case, a, g)[3] for a in AGES}))
        for a in AGES:
            check(gpu_clip(ctx, boxes, counts, a, g, tcap), ref_of(case, a, g), "%s, max_age %d, gain %g" % (case, a, g))


# ------------------------------------------------------------------ 2. gain 0 is dt_associate_mem
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_gain_0_equals_the_memory_entries(case):
    boxes, counts, tcap, chunkings = seq(case)
    cap = boxes.shape[1]
    ctx = ctx_()
    b, c = dev(boxes[None], ctx), dev(counts[None], ctx)
    for a in AGES:
        want = ctx.associate(b, c, THR, max_age=a, track_cap=tcap, want_gaps=True)
        got = ctx.associate(b, c, THR, max_age=a, track_cap=tcap, want_gaps=True, motion_gain=0.0)
        for w, g, what in zip(want, got, ("ids", "nids", "gaps")):
            assert torch.equal(w, g), "%s, max_age %d" % (what, a)
    ctx.stream_open(3, cap, track_cap=tcap)
    for chunks in chunkings:
        ctx.stream_reset([1, 2])
        ids, nid, gaps = gpu_chunked(ctx, boxes, counts, chunks, 1, 3, 0.0)
        mid, mnid, mgaps = gpu_chunked(ctx, boxes, counts, chunks, 2, 3, 0.0, mem_at=range(len(chunks)))
        assert np.array_equal(ids, mid) and nid == mnid and np.array_equal(np.concatenate(gaps), np.concatenate(mgaps)), "chunks %s" % chunks


# ------------------------------------------------------------------ 3. many clips in one call
@pytest.mark.parametrize("tcap", [64, 80])
def test_48_clips_in_one_call(tcap):
    """one wavefront per clip: 48 clips of different seeds in one launch, in the register form (tcap 64) and in the LDS form
    (tcap 80; no entry is cut in either, so one restatement serves both); and d_gaps == NULL"""
    ctx = ctx_()
    T, cap = 10, 32
    if "clips48" not in _REF:
        seqs = [tm.moving_boxes(T, cap, (lambda t, k=k: 6 + k % 7), seed=100 + k) for k in range(48)]
        refs = [tmo.associate_motion(b, c, THR, 3, 0.5, 64) for b, c in seqs]
        assert all(r[3] == 0 for r in refs)
        _REF["clips48"] = (seqs, refs)
    seqs, refs = _REF["clips48"]
    b = np.stack([s[0] for s in seqs]); c = np.stack([s[1] for s in seqs])
    ids, nids, gaps = ctx.associate(dev(b, ctx), dev(c, ctx), THR, max_age=3, track_cap=tcap, want_gaps=True, motion_gain=0.5)
    ids2, nids2 = ctx.associate(dev(b, ctx), dev(c, ctx), THR, max_age=3, track_cap=tcap, motion_gain=0.5)
    assert torch.equal(ids, ids2) and torch.equal(nids, nids2)
    ids, nids, gaps = ids.cpu().numpy(), nids.cpu().numpy(), gaps.cpu().numpy()
    for k in range(48):
        check((ids[k], int(nids[k]), gaps[k]), refs[k], "clip %d" % k)


# ------------------------------------------------------------------ 4. the capacity cut
@pytest.mark.parametrize("form", ["lds", "registers"])
def test_capacity_cut(form):
    """lds: 120 then 20 objects, a table of 140 entries.  registers: 30 objects in frames of at most 32 boxes with a table of 36
    entries -- the cut inside the register form's lane permutation, velocities and all.  (With the tables of the track-memory
    test, 160 and 40, the cut removes entries but no later box would have claimed one of them.)"""
    ctx = ctx_()
    if form == "lds":
        T, cap, n_obj_t, _, _ = tm.CASES["table_over_64_then_small"]
        tcap, roomy = 140, 256
    else:
        T, cap, n_obj_t, tcap, roomy = 40, 32, (lambda t: 30), 36, 64
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    tight = tmo.associate_motion(boxes, counts, THR, 8, 0.5, tcap)
    loose = tmo.associate_motion(boxes, counts, THR, 8, 0.5, roomy)
    print("%s: tcap %d cuts %d entries, tcap %d cuts %d; ids differ in %d places" % (form, tcap, tight[3], roomy, loose[3], int((tight[0] != loose[0]).sum())))
    assert tight[3] > 0 and loose[3] == 0
    assert (tight[0] != loose[0]).any(), "the cut changes no id: the test would not see it"
    got_t, got_l = gpu_clip(ctx, boxes, counts, 8, 0.5, tcap), gpu_clip(ctx, boxes, counts, 8, 0.5, roomy)
    check(got_t, tight, "tcap %d" % tcap)
    check(got_l, loose, "tcap %d" % roomy)


# ------------------------------------------------------------------ 5. chunk invariance for streams
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_stream_chunk_invariance(case):
    boxes, counts, tcap, chunkings = seq(case)
    ctx = ctx_()
    ctx.stream_open(2, boxes.shape[1], track_cap=tcap)
    for a, g in ((3, 0.5), (1, 1.0), (0, 1.0)):
        ref = ref_of(case, a, g)
        for chunks in chunkings:
            ctx.stream_reset([1])
            ids, nid, gaps = gpu_chunked(ctx, boxes, counts, chunks, 1, a, g)
            check((ids, nid, np.concatenate(gaps)), ref, "%s, max_age %d, gain %g, chunks %s" % (case, a, g, chunks))


def test_5_streams_out_of_step():
    """five streams of 8 .. 72 objects advancing by different chunks in shared calls: one call carries tables below and above
    64 live entries; tcap 128 > cap 96"""
    ctx = ctx_()
    n, T, cap, tcap = 5, 24, 96, 128
    seqs = [tm.moving_boxes(T, cap, (lambda t, k=k: 8 + 16 * k), seed=20 + k) for k in range(n)]
    refs = [tmo.associate_motion(b, c, THR, 3, 0.5, tcap) for b, c in seqs]
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
        ids, nids, gaps = ctx.associate_stream(dev(b, ctx), dev(c, ctx), THR, [slot[k] for k in who], max_age=3, want_gaps=True, motion_gain=0.5)
        for j, k in enumerate(who):
            got[k].append(ids[j].cpu().numpy()); gg[k].append(gaps[j].cpu().numpy()); nid[k] = int(nids[j]); cur[k] += L; cuts[k].append(L)
        call += 1
    assert len({tuple(c) for c in cuts}) == n
    for k in range(n):
        check((np.concatenate(got[k]), nid[k], np.concatenate(gg[k])), refs[k], "stream %d (chunks %s)" % (k, cuts[k]))


# ------------------------------------------------------------------ 6. the three stream entries mixed on one slot
@pytest.mark.parametrize("case", ["register_form", "table_over_64_then_small"])
def test_mixed_entries_on_one_slot(case):
    """motion call, dt_associate_stream_mem (or dt_associate_stream), motion call: the middle call runs the memory rule on the
    table the motion call left and makes the tracks forget their velocities"""
    boxes, counts, tcap, _ = seq(case)
    T, cap = boxes.shape[:2]
    ctx = ctx_()
    third = T // 3
    chunks = [third, third, T - 2 * third]
    ctx.stream_open(3, cap, track_cap=tcap)
    unmixed = ref_of(case, 3, 0.5)
    # dt_associate_stream_mem in the middle
    ref = tmo.associate_motion_chunked(boxes, counts, THR, 3, 0.5, tcap, chunks, plain_at=(1,))
    assert not np.array_equal(ref[0], unmixed[0]), "vacuous: forgetting the velocities changes no id"
    ids, nid, gaps = gpu_chunked(ctx, boxes, counts, chunks, 0, 3, 0.5, mem_at=(1,))
    check((ids, nid, np.concatenate(gaps)), ref, "motion, memory, motion")
    # dt_associate_stream in the middle: the memory rule with max_age 0 there
    per_frame = [3] * third + [0] * third + [3] * (T - 2 * third)
    ref = tmo.associate_motion_chunked(boxes, counts, THR, per_frame, 0.5, tcap, chunks, plain_at=(1,))
    ids, nid, gaps = gpu_chunked(ctx, boxes, counts, chunks, 1, 3, 0.5, old_at=(1,))
    assert np.array_equal(ids, ref[0]) and nid == ref[1]
    assert np.array_equal(gaps[0], ref[2][:third]) and np.array_equal(gaps[2], ref[2][2 * third:])


# ------------------------------------------------------------------ 7. slots independent, reset, reopen
def test_slots_independent_reset_and_reopen():
    ctx = ctx_()
    T, cap, tcap = 24, 32, 64
    A = tm.moving_boxes(T, cap, lambda t: 12, seed=7)
    B = tm.moving_boxes(T, cap, lambda t: 14, seed=8)
    refA, refB = (tmo.associate_motion(b, c, THR, 3, 0.5, tcap) for b, c in (A, B))
    refA_head = tmo.associate_motion(A[0][:12], A[1][:12], THR, 3, 0.5, tcap)
    ctx.stream_open(4, cap, track_cap=tcap)

    def call(parts, slots, gain=0.5):
        b = np.stack([p[0] for p in parts]); c = np.stack([p[1] for p in parts])
        ids, nids, gaps = ctx.associate_stream(dev(b, ctx), dev(c, ctx), THR, slots, max_age=3, want_gaps=True, motion_gain=gain)
        return ids.cpu().numpy(), nids.cpu().numpy(), gaps.cpu().numpy()

    cut = lambda s, a, b: (s[0][a:b], s[1][a:b])
    i1, n1, g1 = call([cut(A, 0, 12), cut(B, 0, 12)], [3, 1])
    ctx.stream_reset([3])
    # slot 3 starts over on A's first half (ids from 0, an empty table); slot 1 goes on with B, velocities and all
    i2, n2, g2 = call([cut(B, 12, 24), cut(A, 0, 12)], [1, 3])
    assert np.array_equal(i2[1], refA_head[0]) and n2[1] == refA_head[1] and np.array_equal(g2[1], refA_head[2])
    assert np.array_equal(i1[0], refA_head[0])
    check((np.concatenate([i1[1], i2[0]]), int(n2[0]), np.concatenate([g1[1], g2[0]])), refB, "neighbour of a reset slot")
    i3, n3, g3 = call([cut(A, 12, 24)], [3])
    check((np.concatenate([i2[1], i3[0]]), int(n3[0]), np.concatenate([g2[1], g3[0]])), refA, "the reset slot, continued")
    # a reset slot that then sees as many frames through the memory entry as it had seen through the motion entry: its old
    # velocities must not come back (the frame counter alone would say they are the table's)
    ctx.stream_reset([3])
    b, c = dev(A[0][None, :12], ctx), dev(A[1][None, :12], ctx)
    im, nm, gm = ctx.associate_stream(b, c, THR, [3], max_age=3, want_gaps=True)
    i5, n5, g5 = call([cut(A, 12, 24)], [3])
    ref = tmo.associate_motion_chunked(A[0], A[1], THR, 3, 0.5, tcap, [12, 12], plain_at=(0,))
    check((np.concatenate([im[0].cpu().numpy(), i5[0]]), int(n5[0]), np.concatenate([gm[0].cpu().numpy(), g5[0]])), ref,
          "reset, memory call, motion call")
    assert not np.array_equal(ref[0], refA[0])
    # dt_stream_open again: every slot fresh
    ctx.stream_open(4, cap, track_cap=tcap)
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
    ref = tmo.associate_motion(boxes, counts, THR, 3, 0.5, tcap)
    b = lambda a, z: dev(boxes[None, a:z], ctx)
    c = lambda a, z: dev(counts[None, a:z], ctx)

    fresh = type(trk)(detector_weights=blob, tracker_weights=tw)      # no stream_open yet
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.model.ctx.associate_stream(b(0, 4), c(0, 4), THR, [0], max_age=3, motion_gain=0.5)
    assert _code(e) == STATE
    fresh.model.ctx.close()

    # the stateless entry
    for gain in (-0.1, 1.5, float("nan")):
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate(b(0, 4), c(0, 4), THR, max_age=3, track_cap=tcap, motion_gain=gain)
        assert _code(e) == ARG, gain
    for bad_age, bad_cap in ((-1, 64), (3, 31)):
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate(b(0, 4), c(0, 4), THR, max_age=bad_age, track_cap=bad_cap, motion_gain=0.5)
        assert _code(e) == ARG
    # 2400 entries: 14 words each fit the LDS (the memory entry takes them), 18 do not -- refused, never launched
    ctx.associate(b(0, 4), c(0, 4), THR, max_age=3, track_cap=2400)
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate(b(0, 4), c(0, 4), THR, max_age=3, track_cap=2400, motion_gain=0.5)
    assert _code(e) == ARG
    ctx.stream_open(2, cap, track_cap=2400)
    ctx.associate_stream(b(0, 4), c(0, 4), THR, [0], max_age=3)
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_stream(b(4, 8), c(4, 8), THR, [0], max_age=3, motion_gain=0.5)
    assert _code(e) == ARG

    # the stream entry: refused calls between two valid ones
    ctx.stream_open(4, cap, track_cap=tcap)
    i1, n1, g1 = ctx.associate_stream(b(0, 9), c(0, 9), THR, [2], max_age=3, want_gaps=True, motion_gain=0.5)
    for gain in (-0.1, 1.5, float("nan")):
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_stream(b(9, 20), c(9, 20), THR, [2], max_age=3, motion_gain=gain)
        assert _code(e) == ARG, gain
    for bad in ([4], [-1]):
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_stream(b(9, 20), c(9, 20), THR, bad, max_age=3, motion_gain=0.5)
        assert _code(e) == ARG, bad
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_stream(dev(boxes[None, 9:11].repeat(2, 0), ctx), dev(counts[None, 9:11].repeat(2, 0), ctx), THR, [2, 2], max_age=3,
                             motion_gain=0.5)
    assert _code(e) == ARG
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_stream(b(9, 20), c(9, 20), THR, [2], max_age=-1, motion_gain=0.5)
    assert _code(e) == ARG
    with pytest.raises(mi355_dt.NativeError) as e:      # cap differs from the table's
        ctx.associate_stream(dev(boxes[None, 9:20, :31], ctx), c(9, 20), THR, [2], max_age=3, motion_gain=0.5)
    assert _code(e) == ARG
    n, arr = ctx._slot_array([2])
    assert ctx.lib.dt_associate_stream_motion(ctx.h, None, None, 1, 3, cap, 0.3, 3, 0.5, arr, None, None, None) == ARG
    assert ctx.lib.dt_associate_motion(ctx.h, None, None, 1, 3, cap, 0.3, 3, tcap, 0.5, None, None, None) == ARG
    i2, n2, g2 = ctx.associate_stream(b(9, 20), c(9, 20), THR, [2], max_age=3, want_gaps=True, motion_gain=0.5)
    check((np.concatenate([i1[0].cpu().numpy(), i2[0].cpu().numpy()]), int(n2[0]),
           np.concatenate([g1[0].cpu().numpy(), g2[0].cpu().numpy()])), ref, "after the refused calls")
    mem = tm.associate_memory(boxes, counts, THR, 3, tcap)
    assert not np.array_equal(ref[0][9:], mem[0][9:]), "vacuous: the second chunk does not depend on the velocities"


# ------------------------------------------------------------------ 9. the library exports the entries
def test_library_exports_the_motion_entries():
    import mi355_dt
    out = subprocess.run(["nm", "-D", "--defined-only", mi355_dt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("dt_associate_motion", "dt_associate_stream_motion"):
        assert name in exported and name in mi355_dt.SYMBOLS
    header = open(os.path.join(os.path.dirname(mi355_dt.LIB_PATH), "..", "include", "mi355_dt.h")).read()
    assert "dt_associate_motion(" in header and "dt_associate_stream_motion(" in header
    assert ctx_().lib.dt_abi_version() == 108


# ------------------------------------------------------------------ 10. end to end at 416
def test_end_to_end_416_chunks_equal_clip():
    from parallel import pinned_policy
    trk, blob, tw, fr = big_tracker()

    class Mot(type(trk)):
        MAX_AGE = 3
        MOTION_GAIN = 0.5

    mot = Mot(detector_weights=blob, tracker_weights=tw)
    try:
        keys = ("netout", "boxes", "counts", "ids", "gaps")
        mot.open_streams(2)
        ctx = mot.model.ctx
        with pinned_policy(ctx):
            ctx.profile_reset(); ctx.profile_enable(True)
            ref = mot.track_clips(fr[:1])
            parts, t0 = [], 0
            for L in (12, 6, 12):
                parts.append(mot.track_stream(fr[:1, t0:t0 + L], [1]))
                t0 += L
            ctx.profile_enable(False)
        names = ctx.profile_names()
        assert "associate:motion" in names and "associate:stream_motion" in names
        assert set(ref) == set(keys) | {"nids"}
        for k in keys:
            assert torch.equal(torch.cat([p[k] for p in parts], dim=1), ref[k]), k
        assert torch.equal(parts[-1]["nids"], ref["nids"])
        assert int(ref["counts"].sum()) > 0
        g = ref["gaps"]
        assert int(g.min()) >= -1 and int(g.max()) <= 3
        # the restatement on the boxes the GPU decoded
        b, c = ref["boxes"][0].cpu().numpy(), ref["counts"][0].cpu().numpy()
        r = tmo.associate_motion(b, c, mot.ASSOC_THRESHOLD, 3, 0.5, b.shape[1])
        check((ref["ids"][0].cpu().numpy(), int(ref["nids"][0]), g[0].cpu().numpy()), r, "416, one clip")
    finally:
        mot.model.ctx.close()


def test_motion_gain_none_result_is_todays():
    from parallel import pinned_policy
    trk, blob, tw, fr = big_tracker()
    assert trk.MOTION_GAIN is None

    class Plain(type(trk)):
        MOTION_GAIN = None

    other = Plain(detector_weights=blob, tracker_weights=tw)
    try:
        ctx = other.model.ctx
        with pinned_policy(trk.model.ctx):
            ref = trk.track_clips(fr[:1])
        with pinned_policy(ctx):
            ctx.profile_reset(); ctx.profile_enable(True)
            got = other.track_clips(fr[:1])
            ctx.profile_enable(False)
        names = ctx.profile_names()
        assert "associate:motion" not in names and "associate:stream_motion" not in names
        assert set(ref) == set(got) == {"boxes", "counts", "ids", "nids", "netout"}
        for k in ("boxes", "counts", "ids", "nids"):
            assert torch.equal(ref[k], got[k]), k
    finally:
        other.model.ctx.close()
