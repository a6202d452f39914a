"""GPU suite (-m gpu): track read-out -- hits per track, and per frame the confirmed tracks with the lost ones at their predicted
place.

Ids, gaps, hits and the read-out's integers are integers; its floats are stored values or one float32 multiply and one add, and
decode.hip forms no fused multiply-add.  So everything here is array_equal / torch.equal against the plain restatement
tests/track_readout_ref.py, the float fields through an int32 view (-0.0 and 0.0 differ): no tolerance anywhere.  Both kernel
forms are covered: registers (tcap <= 64 and T <= 64) and LDS (any tcap).
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import track_memory_ref as tm
import track_motion_ref as tmo
import track_readout_ref as tro

from test_gpu_track_memory import big_tracker, dev, small_tracker

pytestmark = pytest.mark.gpu

THR = 0.3
GAIN = 0.5
AGES = (0, 1, 3)
HITS = (1, 3)

_REF = {}


def ctx_():
    return small_tracker()[0].model.ctx


def seq(case, seed=7):
    T, cap, n_obj_t, tcap, chunkings = tm.CASES[case]
    key = ("seq", case, seed)
    if key not in _REF:
        _REF[key] = tm.moving_boxes(T, cap, n_obj_t, seed=seed)
    return _REF[key] + (tcap, chunkings)


def ref_of(case, max_age, min_hits):
    """the restatement on a tm.CASES entry (seed 7, gain 0.5), computed once per (case, max_age) for all the tests that want it:
    min_hits takes no part in the match and filters the read-out only (tests/test_track_readout_cpu.py checks the shortcut)"""
    key = (case, max_age)
    if key not in _REF:
        boxes, counts, tcap, _ = seq(case)
        _REF[key] = tro.associate_tracks(boxes, counts, THR, max_age, GAIN, 1, tcap)
    return tro.with_min_hits(_REF[key], min_hits)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def to_host(r, k=0):
    """clip k of a result dict of the bindings, as the restatement gives it"""
    out = {key: r[key][k].cpu().numpy() for key in tro.KEYS if key != "nids"}
    out["nids"] = int(r["nids"][k])
    return out


def same(got, ref, what, frames=slice(None)):
    """all seven outputs, exactly; `frames`: the frames to compare (nids is compared when all of them are)"""
    for key in ("ids", "gaps", "hits", "track_counts", "track_info"):
        g, r = got[key][frames], ref[key][frames]
        bad = np.nonzero((g != r).reshape(g.shape[0], -1).any(1))[0]
        assert bad.size == 0, "%s: %s differs from the restatement at frames %s" % (what, key, bad[:8])
    g, r = bits(got["tracks"][frames]), bits(ref["tracks"][frames])
    bad = np.nonzero((g != r).reshape(g.shape[0], -1).any(1))[0]
    assert bad.size == 0, "%s: tracks differ (bitwise) from the restatement at frames %s" % (what, bad[:8])
    if frames == slice(None):
        assert got["nids"] == ref["nids"], "%s: %d ids opened, restatement %d" % (what, got["nids"], ref["nids"])


def gpu_clip(ctx, boxes, counts, max_age, min_hits, tcap, gain=GAIN):
    return to_host(ctx.associate_tracks(dev(boxes[None], ctx), dev(counts[None], ctx), THR, max_age, gain, min_hits, track_cap=tcap))


def join(parts):
    r = {key: np.concatenate([p[key] for p in parts]) for key in tro.KEYS if key != "nids"}
    r["nids"] = parts[-1]["nids"]
    return r


def blank(ids, nid, gaps, tcap):
    """a chunk that went through an entry without hits and read-out, in the restatement's terms (gaps None: zeros, not compared)"""
    T, cap = ids.shape
    return dict(ids=ids, nids=nid, gaps=gaps if gaps is not None else np.zeros_like(ids), hits=np.full((T, cap), -1, np.int32),
                tracks=np.zeros((T, tcap, 8), np.float32), track_info=np.full((T, tcap, 4), -1, np.int32),
                track_counts=np.zeros(T, np.int32))


def gpu_chunked(ctx, boxes, counts, chunks, slot, max_age, min_hits, tcap, motion_at=(), mem_at=(), old_at=()):
    """one stream through slot `slot`; chunks whose index is in motion_at go through dt_associate_stream_motion, those in mem_at
    through dt_associate_stream_mem, those in old_at through dt_associate_stream (no gaps); such chunks come back blank()"""
    parts, t0 = [], 0
    for k, L in enumerate(chunks):
        b, c = dev(boxes[None, t0:t0 + L], ctx), dev(counts[None, t0:t0 + L], ctx)
        if k in old_at:
            i, nid = ctx.associate_stream(b, c, THR, [slot])
            parts.append(blank(i[0].cpu().numpy(), int(nid[0]), None, tcap))
        elif k in mem_at or k in motion_at:
            i, nid, g = ctx.associate_stream(b, c, THR, [slot], max_age=max_age, want_gaps=True, motion_gain=GAIN if k in motion_at else None)
            parts.append(blank(i[0].cpu().numpy(), int(nid[0]), g[0].cpu().numpy(), tcap))
        else:
            parts.append(to_host(ctx.associate_stream_tracks(b, c, THR, [slot], max_age, GAIN, min_hits)))
        t0 += L
    assert t0 == boxes.shape[0]
    return join(parts)


def raw_tracks(ctx, b, c, max_age, tcap, gain, min_hits, gaps=True, hits=True, tracks=True, tinfo=True, tcounts=True, slots=None):
    """the C entries with any of the optional outputs NULL -> (return code, dict of the outputs given)"""
    import mi355_dt
    n, T, cap, _ = b.shape
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=ctx.device)
    o = dict(ids=i32(n, T, cap), nids=i32(n), gaps=i32(n, T, cap) if gaps else None, hits=i32(n, T, cap) if hits else None,
             tracks=torch.full((n, T, tcap, 8), -7.0, device=ctx.device) if tracks else None,
             track_info=i32(n, T, tcap, 4) if tinfo else None, track_counts=i32(n, T) if tcounts else None)
    p = lambda k: mi355_dt._dptr(o[k])
    ctx._sync_stream()
    if slots is None:
        rc = ctx.lib.dt_associate_tracks(ctx.h, mi355_dt._dptr(b), mi355_dt._dptr(c), n, T, cap, THR, max_age, tcap, gain, min_hits,
                                         p("ids"), p("nids"), p("gaps"), p("hits"), p("tracks"), p("track_info"), p("track_counts"))
    else:
        ns, arr = ctx._slot_array(slots)
        rc = ctx.lib.dt_associate_stream_tracks(ctx.h, mi355_dt._dptr(b), mi355_dt._dptr(c), n, T, cap, THR, max_age, gain, min_hits, arr,
                                                p("ids"), p("nids"), p("gaps"), p("hits"), p("tracks"), p("track_info"), p("track_counts"))
    return rc, o


# ------------------------------------------------------------------ 1. parity of all seven outputs with the restatement
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_parity_with_restatement(case):
    boxes, counts, tcap, _ = seq(case)
    T = boxes.shape[0]
    ctx = ctx_()
    register_form = "register" in case or case == "empty_frames"
    assert register_form == (tcap <= 64 and T <= 64)      # which form the launcher takes, from tcap and T alone
    if "over_64" in case:
        assert counts.max() > 64 and counts.min() <= 64
    for a in AGES:
        for m in HITS:
            ref = ref_of(case, a, m)
            if a > 0:
                coasting = (ref["track_info"][..., 3] == -1) & (ref["track_info"][..., 0] >= 0)
                assert coasting.any(), "vacuous: no coasting row (max_age %d, min_hits %d)" % (a, m)
            same(gpu_clip(ctx, boxes, counts, a, m, tcap), ref, "%s, max_age %d, min_hits %d" % (case, a, m))


# ------------------------------------------------------------------ 2. the match is untouched
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_match_is_the_motion_entrys(case):
    boxes, counts, tcap, _ = seq(case)
    ctx = ctx_()
    b, c = dev(boxes[None], ctx), dev(counts[None], ctx)
    for a in AGES:
        for g in (GAIN, 1.0, 0.0):
            want = ctx.associate(b, c, THR, max_age=a, track_cap=tcap, want_gaps=True, motion_gain=g)
            for m in HITS:
                got = ctx.associate_tracks(b, c, THR, a, g, m, track_cap=tcap)
                for w, k in zip(want, ("ids", "nids", "gaps")):
                    assert torch.equal(w, got[k]), "%s, max_age %d, gain %g, min_hits %d" % (k, a, g, m)
        mem = ctx.associate(b, c, THR, max_age=a, track_cap=tcap, want_gaps=True)
        got = ctx.associate_tracks(b, c, THR, a, 0.0, 1, track_cap=tcap)
        for w, k in zip(mem, ("ids", "nids", "gaps")):
            assert torch.equal(w, got[k]), "gain 0 against the memory entry: %s, max_age %d" % (k, a)
        # gain 0: coasting rows stand where the track was last seen, at rest
        assert not got["tracks"][..., 5:7].any()
    # optional outputs NULL: the others are unchanged
    full = ctx.associate_tracks(b, c, THR, 3, GAIN, 3, track_cap=tcap)
    for off in (dict(gaps=False), dict(hits=False), dict(gaps=False, hits=False), dict(tracks=False, tinfo=False, tcounts=False),
                dict(gaps=False, hits=False, tracks=False, tinfo=False, tcounts=False)):
        rc, o = raw_tracks(ctx, b, c, 3, tcap, GAIN, 3, **off)
        assert rc == 0, off
        for k, v in o.items():
            if v is not None:
                if k == "tracks":
                    assert torch.equal(v.view(torch.int32), full[k].view(torch.int32)), (off, k)
                else:
                    assert torch.equal(v, full[k]), (off, k)


# ------------------------------------------------------------------ 3. min_hits = 1, max_age = 0: the read-out is the frame's boxes
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_min_hits_1_max_age_0_reads_out_the_boxes(case):
    boxes, counts, tcap, _ = seq(case)
    T, cap = boxes.shape[:2]
    ctx = ctx_()
    r = gpu_clip(ctx, boxes, counts, 0, 1, tcap)
    n = np.minimum(counts, cap)
    assert np.array_equal(r["track_counts"], n)
    if case == "empty_frames":
        assert (n == 0).any() and (r["track_counts"][n == 0] == 0).all()
    for t in range(T):
        k = int(n[t])
        assert np.array_equal(bits(r["tracks"][t, :k, :4]), bits(boxes[t, :k, :4])), t
        assert np.array_equal(bits(r["tracks"][t, :k, 4]), bits(boxes[t, :k, 5])), t
        assert np.array_equal(r["track_info"][t, :k, 3], np.arange(k)), t
        assert np.array_equal(r["track_info"][t, :k, 0], r["ids"][t, :k]) and (r["track_info"][t, :k, 1] == 0).all()
        assert np.array_equal(r["track_info"][t, :k, 2], r["hits"][t, :k])
        assert (bits(r["tracks"][t, k:]) == 0).all() and (r["track_info"][t, k:] == -1).all()


# ------------------------------------------------------------------ 4. many clips in one call
@pytest.mark.parametrize("tcap", [64, 80])
def test_48_clips_in_one_call(tcap):
    """one wavefront per clip: 48 clips of different seeds in one launch, in the register form (tcap 64) and in the LDS form
    (tcap 80; no entry is cut in either, so one match serves both -- the read-out is laid out again for the wider rows)"""
    ctx = ctx_()
    T, cap = 10, 32
    if "clips48" not in _REF:
        seqs = [tm.moving_boxes(T, cap, (lambda t, k=k: 6 + k % 7), seed=100 + k) for k in range(48)]
        refs = [tro.associate_tracks(b, c, THR, 3, GAIN, 2, 64) for b, c in seqs]
        assert all(r["dropped"] == 0 for r in refs)
        _REF["clips48"] = (seqs, refs)
    seqs, refs = _REF["clips48"]
    b = np.stack([s[0] for s in seqs]); c = np.stack([s[1] for s in seqs])
    got = ctx.associate_tracks(dev(b, ctx), dev(c, ctx), THR, 3, GAIN, 2, track_cap=tcap)
    assert got["tracks"].shape == (48, T, tcap, 8) and got["track_info"].shape == (48, T, tcap, 4)
    for k in range(48):
        ref = dict(refs[k])
        ref.update(tro.read_out(refs[k]["table"], 2, tcap))
        same(to_host(got, k), ref, "clip %d" % k)


# ------------------------------------------------------------------ 5. the capacity cut
@pytest.mark.parametrize("form", ["lds", "registers"])
def test_capacity_cut(form):
    """the motion suite's shapes.  lds: 120 then 20 objects, a table of 140 entries.  registers: 30 objects in frames of at most
    32 boxes with a table of 36 entries -- the cut inside the register form's lane permutation, hits and all"""
    ctx = ctx_()
    if form == "lds":
        T, cap, n_obj_t, _, _ = tm.CASES["table_over_64_then_small"]
        tcap = 140
    else:
        T, cap, n_obj_t, tcap = 40, 32, (lambda t: 30), 36
    assert (form == "registers") == (tcap <= 64 and T <= 64)
    boxes, counts = tm.moving_boxes(T, cap, n_obj_t, seed=7)
    tight = tro.associate_tracks(boxes, counts, THR, 8, GAIN, 2, tcap)
    print("%s: tcap %d cuts %d entries; fullest read-out %d rows" % (form, tcap, tight["dropped"], int(tight["track_counts"].max())))
    assert tight["dropped"] > 0
    assert max(len(rows) for rows in tight["table"]) == tcap, "the table is never full"
    same(gpu_clip(ctx, boxes, counts, 8, 2, tcap), tight, "tcap %d" % tcap)
    same(gpu_clip(ctx, boxes, counts, 8, 1, tcap), tro.with_min_hits(tight, 1), "tcap %d, min_hits 1" % tcap)


# ------------------------------------------------------------------ 6. streams
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_stream_chunk_invariance(case):
    boxes, counts, tcap, chunkings = seq(case)
    T = boxes.shape[0]
    ctx = ctx_()
    ctx.stream_open(2, boxes.shape[1], track_cap=tcap)
    for a, m, more in ((3, 3, [[1] * T]), (1, 1, [])):
        ref = ref_of(case, a, m)
        for chunks in chunkings + [ch for ch in more if ch not in chunkings]:
            ctx.stream_reset([1])
            got = gpu_chunked(ctx, boxes, counts, chunks, 1, a, m, tcap)
            same(got, ref, "%s, max_age %d, min_hits %d, chunks %s" % (case, a, m, chunks))


def test_5_streams_out_of_step():
    """five streams of 8 .. 72 objects advancing by different chunks in shared calls: one call carries tables below and above
    64 live entries; tcap 128 > cap 96"""
    ctx = ctx_()
    n, T, cap, tcap = 5, 24, 96, 128
    seqs = [tm.moving_boxes(T, cap, (lambda t, k=k: 8 + 16 * k), seed=20 + k) for k in range(n)]
    refs = [tro.associate_tracks(b, c, THR, 3, GAIN, 2, tcap) for b, c in seqs]
    live = [max(len(rows) for rows in r["table"]) for r in refs]
    assert min(live) < 64 < max(live)
    slot = [6, 0, 3, 8, 1]
    ctx.stream_open(9, cap, track_cap=tcap)
    cur, got, call = [0] * n, [[] for _ in range(n)], 0
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
        r = ctx.associate_stream_tracks(dev(b, ctx), dev(c, ctx), THR, [slot[k] for k in who], 3, GAIN, 2)
        for j, k in enumerate(who):
            got[k].append(to_host(r, j)); cur[k] += L; cuts[k].append(L)
        call += 1
    assert len({tuple(c) for c in cuts}) == n
    for k in range(n):
        same(join(got[k]), refs[k], "stream %d (chunks %s)" % (k, cuts[k]))


@pytest.mark.parametrize("case", ["register_form", "table_over_64_then_small"])
def test_mixed_entries_on_one_slot(case):
    """read-out call, another stream entry, read-out call.  Through dt_associate_stream_motion the match goes on and the hits
    are forgotten; through dt_associate_stream_mem / dt_associate_stream the velocities are forgotten too"""
    boxes, counts, tcap, _ = seq(case)
    T, cap = boxes.shape[:2]
    ctx = ctx_()
    third = T // 3
    chunks = [third, third, T - 2 * third]
    outer = [t for t in range(T) if not third <= t < 2 * third]
    ctx.stream_open(3, cap, track_cap=tcap)
    unmixed = ref_of(case, 3, 2)
    # dt_associate_stream_motion in the middle
    ref = tro.associate_tracks_chunked(boxes, counts, THR, 3, GAIN, 2, tcap, chunks, motion_at=(1,))
    assert np.array_equal(ref["ids"], unmixed["ids"]) and not np.array_equal(ref["hits"][2 * third:], unmixed["hits"][2 * third:])
    assert not np.array_equal(ref["track_counts"][2 * third:], unmixed["track_counts"][2 * third:]), "vacuous: forgetting the hits changes no row"
    got = gpu_chunked(ctx, boxes, counts, chunks, 0, 3, 2, tcap, motion_at=(1,))
    same(got, ref, "read-out, motion, read-out")
    # dt_associate_stream_mem in the middle
    ref = tro.associate_tracks_chunked(boxes, counts, THR, 3, GAIN, 2, tcap, chunks, plain_at=(1,))
    assert not np.array_equal(ref["ids"], unmixed["ids"]), "vacuous: forgetting the velocities changes no id"
    got = gpu_chunked(ctx, boxes, counts, chunks, 1, 3, 2, tcap, mem_at=(1,))
    same(got, ref, "read-out, memory, read-out")
    # dt_associate_stream in the middle: the memory rule with max_age 0 there, and no gaps from it
    per_frame = [3] * third + [0] * third + [3] * (T - 2 * third)
    ref = tro.associate_tracks_chunked(boxes, counts, THR, per_frame, GAIN, 2, tcap, chunks, plain_at=(1,))
    got = gpu_chunked(ctx, boxes, counts, chunks, 2, 3, 2, tcap, old_at=(1,))
    assert np.array_equal(got["ids"], ref["ids"]) and got["nids"] == ref["nids"]
    same(got, ref, "read-out, dt_associate_stream, read-out", frames=outer)


def test_slots_independent_reset_and_reopen():
    ctx = ctx_()
    T, cap, tcap = 24, 32, 64
    A = tm.moving_boxes(T, cap, lambda t: 12, seed=7)
    B = tm.moving_boxes(T, cap, lambda t: 14, seed=8)
    refA, refB = (tro.associate_tracks(b, c, THR, 3, GAIN, 2, tcap) for b, c in (A, B))
    refA_head = tro.associate_tracks(A[0][:12], A[1][:12], THR, 3, GAIN, 2, tcap)
    ctx.stream_open(4, cap, track_cap=tcap)

    def call(parts, slots):
        b = np.stack([p[0] for p in parts]); c = np.stack([p[1] for p in parts])
        r = ctx.associate_stream_tracks(dev(b, ctx), dev(c, ctx), THR, slots, 3, GAIN, 2)
        return [to_host(r, k) for k in range(len(parts))]

    cut = lambda s, a, b: (s[0][a:b], s[1][a:b])
    a1, b1 = call([cut(A, 0, 12), cut(B, 0, 12)], [3, 1])
    same(a1, refA_head, "slot 3, first half")
    ctx.stream_reset([3])
    # slot 3 starts over on A's first half (ids from 0, an empty table, no hits); slot 1 goes on with B, velocities, hits and all
    b2, a2 = call([cut(B, 12, 24), cut(A, 0, 12)], [1, 3])
    same(a2, refA_head, "the reset slot")
    same(join([b1, b2]), refB, "neighbour of a reset slot")
    a3, = call([cut(A, 12, 24)], [3])
    same(join([a2, a3]), refA, "the reset slot, continued")
    # a reset slot that then sees as many frames through the motion entry as it had seen through this one: its old hits must not
    # come back (the frame counter alone would say they are the table's)
    ctx.stream_reset([3])
    ref = tro.associate_tracks_chunked(A[0], A[1], THR, 3, GAIN, 2, tcap, [12, 12], motion_at=(0,))
    got = gpu_chunked(ctx, A[0], A[1], [12, 12], 3, 3, 2, tcap, motion_at=(0,))
    same(got, ref, "reset, motion call, read-out call")
    assert not np.array_equal(ref["hits"][12:], refA["hits"][12:])
    # dt_stream_open again: every slot fresh
    ctx.stream_open(4, cap, track_cap=tcap)
    a4, b4 = call([cut(A, 0, 12), cut(B, 0, 12)], [3, 1])
    same(a4, a1, "reopened, slot 3"); same(b4, b1, "reopened, slot 1")


# ------------------------------------------------------------------ 7. errors
def _code(excinfo):
    return int(re.search(r"failed \((\d+)\)", str(excinfo.value)).group(1))


def test_errors_leave_the_state_unchanged():
    import mi355_dt
    trk, blob, tw = small_tracker()
    ctx = trk.model.ctx
    ARG, STATE = 1, 3
    T, cap, tcap = 20, 32, 64
    boxes, counts = tm.moving_boxes(T, cap, lambda t: 12, seed=7)
    ref = tro.associate_tracks(boxes, counts, THR, 3, GAIN, 2, tcap)
    b = lambda a, z: dev(boxes[None, a:z], ctx)
    c = lambda a, z: dev(counts[None, a:z], ctx)
    partial = (dict(tracks=False), dict(tinfo=False), dict(tcounts=False), dict(tracks=False, tinfo=False), dict(tinfo=False, tcounts=False),
               dict(tracks=False, tcounts=False))

    fresh = type(trk)(detector_weights=blob, tracker_weights=tw)      # no stream_open yet
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.model.ctx.associate_stream_tracks(b(0, 4), c(0, 4), THR, [0], 3, GAIN, 2)
    assert _code(e) == STATE
    fresh.model.ctx.close()

    # the stateless entry
    for bad in (dict(min_hits=0), dict(min_hits=-1), dict(gain=1.5), dict(gain=-0.1), dict(gain=float("nan")), dict(max_age=-1),
                dict(track_cap=31)):
        kw = dict(max_age=3, gain=GAIN, min_hits=2, track_cap=tcap)
        kw.update(bad)
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_tracks(b(0, 4), c(0, 4), THR, kw["max_age"], kw["gain"], kw["min_hits"], track_cap=kw["track_cap"])
        assert _code(e) == ARG, bad
    for off in partial:
        assert raw_tracks(ctx, b(0, 4), c(0, 4), 3, tcap, GAIN, 2, **off)[0] == ARG, off
    # 2200 entries: 18 words each fit the LDS (the motion entry takes them), 20 do not -- refused, never launched
    ctx.associate(b(0, 4), c(0, 4), THR, max_age=3, track_cap=2200, motion_gain=GAIN)
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_tracks(b(0, 4), c(0, 4), THR, 3, GAIN, 2, track_cap=2200)
    assert _code(e) == ARG
    ctx.stream_open(2, cap, track_cap=2200)
    i1, _ = ctx.associate_stream(b(0, 4), c(0, 4), THR, [0], max_age=3, motion_gain=GAIN)
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_stream_tracks(b(4, 8), c(4, 8), THR, [0], 3, GAIN, 2)
    assert _code(e) == ARG
    i2, n2 = ctx.associate_stream(b(4, 8), c(4, 8), THR, [0], max_age=3, motion_gain=GAIN)
    want = tmo.associate_motion(boxes[:8], counts[:8], THR, 3, GAIN, 2200)
    assert np.array_equal(torch.cat([i1[0], i2[0]]).cpu().numpy(), want[0]) and int(n2[0]) == want[1]

    # the stream entry: refused calls between two valid ones
    ctx.stream_open(4, cap, track_cap=tcap)
    r1 = to_host(ctx.associate_stream_tracks(b(0, 9), c(0, 9), THR, [2], 3, GAIN, 2))
    for bad in (dict(min_hits=0), dict(gain=1.5), dict(gain=float("nan")), dict(max_age=-1), dict(slots=[4]), dict(slots=[-1])):
        kw = dict(max_age=3, gain=GAIN, min_hits=2, slots=[2])
        kw.update(bad)
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_stream_tracks(b(9, 20), c(9, 20), THR, kw["slots"], kw["max_age"], kw["gain"], kw["min_hits"])
        assert _code(e) == ARG, bad
    for off in partial:
        assert raw_tracks(ctx, b(9, 20), c(9, 20), 3, tcap, GAIN, 2, slots=[2], **off)[0] == ARG, off
    with pytest.raises(mi355_dt.NativeError) as e:      # a slot named twice
        ctx.associate_stream_tracks(dev(boxes[None, 9:11].repeat(2, 0), ctx), dev(counts[None, 9:11].repeat(2, 0), ctx), THR, [2, 2], 3, GAIN, 2)
    assert _code(e) == ARG
    with pytest.raises(mi355_dt.NativeError) as e:      # cap differs from the table's
        ctx.associate_stream_tracks(dev(boxes[None, 9:20, :31], ctx), c(9, 20), THR, [2], 3, GAIN, 2)
    assert _code(e) == ARG
    n, arr = ctx._slot_array([2])
    assert ctx.lib.dt_associate_stream_tracks(ctx.h, None, None, 1, 3, cap, 0.3, 3, 0.5, 2, arr, None, None, None, None, None, None, None) == ARG
    assert ctx.lib.dt_associate_tracks(ctx.h, None, None, 1, 3, cap, 0.3, 3, tcap, 0.5, 2, None, None, None, None, None, None, None) == ARG
    r2 = to_host(ctx.associate_stream_tracks(b(9, 20), c(9, 20), THR, [2], 3, GAIN, 2))
    same(join([r1, r2]), ref, "after the refused calls")
    alone = tro.associate_tracks(boxes[9:], counts[9:], THR, 3, GAIN, 2, tcap)
    assert not np.array_equal(ref["hits"][9:], alone["hits"]), "vacuous: the second chunk does not depend on the slot"


# ------------------------------------------------------------------ 8. the library exports the entries
def test_library_exports_the_track_entries():
    import mi355_dt
    out = subprocess.run(["nm", "-D", "--defined-only", mi355_dt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("dt_associate_tracks", "dt_associate_stream_tracks"):
        assert name in exported and name in mi355_dt.SYMBOLS
    header = open(os.path.join(os.path.dirname(mi355_dt.LIB_PATH), "..", "include", "mi355_dt.h")).read()
    assert "dt_associate_tracks(" in header and "dt_associate_stream_tracks(" in header
    assert ctx_().lib.dt_abi_version() == 108


# ------------------------------------------------------------------ 9. end to end at 416
def test_end_to_end_416():
    from parallel import pinned_policy
    trk, blob, tw, fr = big_tracker()
    assert trk.MIN_HITS is None

    class Mot(type(trk)):
        MAX_AGE = 2
        MOTION_GAIN = 0.5
        MIN_HITS = 2

    mot = Mot(detector_weights=blob, tracker_weights=tw)
    try:
        keys = ("netout", "boxes", "counts", "ids", "gaps", "hits", "tracks", "track_info", "track_counts")
        mot.open_streams(4)
        ctx = mot.model.ctx
        with pinned_policy(ctx):
            ctx.profile_reset(); ctx.profile_enable(True)
            ref = mot.track_clips(fr)
            ctx.profile_enable(False)
            names = ctx.profile_names()
            assert "associate:tracks" in names and "associate:motion" not in names
            assert set(ref) == set(keys) | {"nids"}
            n_clips, T, cap = ref["ids"].shape
            assert (n_clips, T) == (2, 30) and ref["tracks"].shape == (2, T, cap, 8)
            # the restatement on the boxes the GPU decoded
            for k in range(n_clips):
                b, c = ref["boxes"][k].cpu().numpy(), ref["counts"][k].cpu().numpy()
                same(to_host(ref, k), tro.associate_tracks(b, c, mot.ASSOC_THRESHOLD, 2, 0.5, 2, cap), "416, clip %d" % k)
            info = ref["track_info"]
            assert int(ref["counts"].sum()) > 0 and int(ref["track_counts"].sum()) > 0
            assert bool(((info[..., 3] == -1) & (info[..., 0] >= 0)).any()), "no coasting row at 416"
            # streams in chunks
            for slots, chunks in (([1, 3], [7, 23]), ([0, 2], [1] * 30)):
                ctx.profile_reset(); ctx.profile_enable(True)
                parts, t0 = [], 0
                for L in chunks:
                    parts.append(mot.track_stream(fr[:, t0:t0 + L], slots))
                    t0 += L
                ctx.profile_enable(False)
                assert "associate:stream_tracks" in ctx.profile_names()
                for key in keys:
                    got = torch.cat([p[key] for p in parts], dim=1)
                    assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                                       ref[key].view(torch.int32) if got.dtype == torch.float32 else ref[key]), (chunks, key)
                assert torch.equal(parts[-1]["nids"], ref["nids"]), chunks
            # the host views
            for k in range(n_clips):
                per_t = mot.tracks_from_result(ref, k)
                frames = mot.boxes_from_result(ref, k)
                tr, inf, tc = (ref[key][k].cpu().numpy() for key in ("tracks", "track_info", "track_counts"))
                bx, hits = ref["boxes"][k].cpu().numpy(), ref["hits"][k].cpu().numpy()
                assert [len(l) for l in per_t] == tc.tolist()
                for t in range(T):
                    assert [bb.track_hits for bb in frames[t]] == hits[t, :len(frames[t])].tolist()
                    for j, bb in enumerate(per_t[t]):
                        assert [bb.x, bb.y, bb.w, bb.h] == tr[t, j, :4].tolist() and bb.label == int(tr[t, j, 4])
                        assert (bb.track_id, bb.track_age, bb.track_hits) == tuple(inf[t, j, :3])
                        i = inf[t, j, 3]
                        assert (bb.c, bb.score) == ((bx[t, i, 4], bx[t, i, 6]) if i >= 0 else (0.0, 0.0))
                        assert (i >= 0) == (bb.track_age == 0)
            # MIN_HITS = None: today's result
            mot.MIN_HITS = None
            ctx.profile_reset(); ctx.profile_enable(True)
            plain = mot.track_clips(fr)
            ctx.profile_enable(False)
            names = ctx.profile_names()
            assert "associate:motion" in names and "associate:tracks" not in names
            assert set(plain) == {"boxes", "counts", "ids", "nids", "gaps", "netout"}
            want = ctx.associate(plain["boxes"], plain["counts"], mot.ASSOC_THRESHOLD, max_age=2, want_gaps=True, motion_gain=0.5)
            for key, w in zip(("ids", "nids", "gaps"), want):
                assert torch.equal(plain[key], w) and torch.equal(plain[key], ref[key]), key
            for key in ("boxes", "counts", "netout"):
                assert torch.equal(plain[key], ref[key]), key
            assert all(bb.track_hits is None for l in mot.boxes_from_result(plain, 0) for bb in l)
            e = mot.empty_result(T)
            assert set(e) == {"boxes", "counts", "ids", "nids", "netout"}
            mot.MIN_HITS = 2
            e = mot.empty_result(T)
            assert set(e) == set(keys) | {"nids"}
            assert all(e[key].shape[0] == 0 and e[key].shape[1:] == ref[key].shape[1:] and e[key].dtype == ref[key].dtype
                       for key in keys if key != "netout")
    finally:
        mot.model.ctx.close()
