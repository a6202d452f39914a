"""GPU suite (-m gpu): track scores -- the two-pass match that uses the detection score beside each box (DESIGN.md section 6,
dt_associate_tracks_scored and its stream entry).

Everything is compared exactly with the plain restatement tests/track_scored_ref.py, floats through an int32 view.  Both kernel
forms are covered -- registers (tcap <= 64 and T <= 64) and LDS (by tcap, by T) -- at the shapes of track_assign_ref.SCENES,
three clips per call (the score seeds 11, 12, 13), so that several wavefronts run.
"""
import re

import numpy as np
import pytest
import torch

import track_assign_ref as tar
import track_scored_ref as tsr

from test_gpu_track_memory import dev, small_tracker
from test_gpu_track_readout import blank, join, same, to_host

pytestmark = pytest.mark.gpu

THR, GAIN = tsr.THR, tsr.GAIN
BEST, ANY = tsr.MATCH_BEST_FIRST, tsr.MATCH_ANY_LABEL
SCENES = sorted(tsr.SCENES)
SEEDS = tsr.SCORE_SEEDS
CHUNKS = {"crowd_reg_grow": [1, 4, 7], "crowd_reg": [1, 4, 7], "crowd_lds": [2, 1, 3], "crowd_long": [30, 36]}
ARG = 1


def ctx_():
    return small_tracker()[0].model.ctx


def clips(name):
    """the scene under the three score seeds -> (boxes [3, T, cap, 8], counts [3, T], tcap, max_age)"""
    pairs = [tsr.scene(name, s) for s in SEEDS]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), tsr.SCENES[name][3], tsr.SCENES[name][4]


def scored(ctx, boxes, counts, max_age, min_hits, tcap, match, **score):
    kw = dict(score_high=tsr.SCORE_HIGH, score_new=tsr.SCORE_NEW, assoc_threshold_low=tsr.THR_LOW, max_age_low=tsr.MAX_AGE_LOW,
              score_at=tsr.SCORE_AT)
    kw.update(score)
    return ctx.associate_tracks_scored(dev(boxes, ctx), dev(counts, ctx), THR, max_age, GAIN, min_hits, track_cap=tcap, match=match, **kw)


def ref_kw(score):
    """the binding's keyword names -> the restatement's"""
    return {dict(assoc_threshold_low="thr_low").get(k, k): v for k, v in score.items()}


def check_tables(got, what):
    """no read-out row is a dead one; an age-0 row's `box` indexes a box that carries the row's id"""
    info, n = got["track_info"], got["track_counts"]
    for t in range(info.shape[0]):
        rows = info[t, :n[t]]
        assert (rows[:, 0] >= 0).all() and (rows[:, 2] >= 1).all(), "%s: a dead row was read out in frame %d" % (what, t)
        now = rows[rows[:, 1] == 0]
        assert (now[:, 3] >= 0).all() and np.array_equal(got["ids"][t, now[:, 3]], now[:, 0]), "%s: frame %d" % (what, t)


# ------------------------------------------------------------------ 1. parity of all seven outputs with the restatement
@pytest.mark.parametrize("match", [0, ANY])
@pytest.mark.parametrize("name", SCENES)
def test_parity_with_restatement(name, match):
    boxes, counts, tcap, max_age = clips(name)
    T, cap = boxes.shape[1:3]
    assert tar.form_of(tcap, T) == tsr.SCENES[name][7]
    ctx = ctx_()
    for min_hits in (1, 3):
        got = scored(ctx, boxes, counts, max_age, min_hits, tcap, match)
        for k, seed in enumerate(SEEDS):
            ref = tsr.scene_ref(name, match, min_hits, seed)
            assert ref["stats"]["pass2"] >= 20 and ref["stats"]["dropped_boxes"] >= 50 and ref["dropped"] == 0
            what = "%s, match %d, min_hits %d, seed %d" % (name, match, min_hits, seed)
            same(to_host(got, k), ref, what)
            check_tables(to_host(got, k), what)


# ------------------------------------------------------------------ 2. the smallest case
def test_worked_example():
    ctx = ctx_()
    boxes, counts = tsr.worked_example()
    for tcap in (2, 80):
        for any_label in (0, ANY):
            got = to_host(scored(ctx, boxes[None], counts[None], 0, 1, tcap, any_label))
            assert got["ids"].tolist() == [[0, -1], [-1, 0], [0, -1]] and got["nids"] == 1, tcap
            assert got["hits"].tolist() == [[1, -1], [0, 2], [3, -1]] and got["gaps"].tolist() == [[-1, -1], [-1, 0], [0, -1]], tcap
            same(got, tsr.associate_tracks_scored(boxes, counts, THR, 0, GAIN, 1, any_label, tcap), "tcap %d" % tcap)
            b, c = dev(boxes[None], ctx), dev(counts[None], ctx)
            assert int(ctx.associate_tracks(b, c, THR, 0, GAIN, 1, track_cap=tcap, match=any_label, assign=True)["nids"][0]) == 2


# ------------------------------------------------------------------ 3. the equivalences, on the device
@pytest.mark.parametrize("name", ["crowd_reg", "crowd_lds", "crowd_long"])
def test_all_boxes_confident_is_the_plain_assignment(name):
    boxes, counts, tcap, max_age = clips(name)
    ctx = ctx_()
    for match in (0, ANY):
        got = scored(ctx, boxes, counts, max_age, 2, tcap, match, score_high=0.0, score_new=0.0)
        want = ctx.associate_tracks(dev(boxes, ctx), dev(counts, ctx), THR, max_age, GAIN, 2, track_cap=tcap, match=match, assign=True)
        for key in tsr.KEYS:
            g, w = got[key], want[key]
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w), (match, key)
    lo = scored(ctx, boxes, counts, max_age, 2, tcap, 0, score_high=-1.0, score_new=-1.0, max_age_low=-1, assoc_threshold_low=0.9)
    plain0 = ctx.associate_tracks(dev(boxes, ctx), dev(counts, ctx), THR, max_age, GAIN, 2, track_cap=tcap, match=0, assign=True)
    for key in ("ids", "nids", "gaps", "hits", "track_info", "track_counts"):
        assert torch.equal(lo[key], plain0[key]), key      # the parameters of the second pass mean nothing when no box is LOW


@pytest.mark.parametrize("name", ["crowd_reg_grow", "crowd_long"])
def test_without_the_second_pass_the_weak_boxes_are_not_there(name):
    boxes, counts, tcap, max_age = clips(name)
    match = tsr.SCENES[name][6]
    ctx = ctx_()
    got = scored(ctx, boxes, counts, max_age, 1, tcap, match, score_new=tsr.SCORE_HIGH, max_age_low=-1)
    packed = [tsr.compact_high(boxes[k], counts[k], tsr.SCORE_HIGH) for k in range(len(SEEDS))]
    want = ctx.associate_tracks(dev(np.stack([p[0] for p in packed]), ctx), dev(np.stack([p[1] for p in packed]), ctx), THR, max_age, GAIN, 1,
                                track_cap=tcap, match=match, assign=True)
    for k in range(len(SEEDS)):
        g, w, index = to_host(got, k), to_host(want, k), packed[k][2]
        assert g["nids"] == w["nids"]
        high = index >= 0
        used = np.arange(index.shape[1])[None, :] < counts[k][:, None]
        assert 0 < high.sum() < used.sum()
        for key, none in (("ids", -1), ("gaps", -1), ("hits", 0)):
            t, i = np.nonzero(high)
            assert np.array_equal(g[key][t, i], w[key][t, index[t, i]]), (k, key)
            assert (g[key][used & ~high] == none).all(), (k, key)


# ------------------------------------------------------------------ 4. every parameter reaches the kernel
def test_parameters():
    name = "crowd_reg"
    boxes, counts, tcap, max_age = clips(name)
    ctx = ctx_()
    base = tsr.scene_ref(name, 0)
    for score in (dict(max_age_low=2), dict(assoc_threshold_low=0.5), dict(max_age_low=1, score_new=0.3, score_high=0.7)):
        got = scored(ctx, boxes, counts, max_age, 1, tcap, 0, **score)
        for k, seed in enumerate(SEEDS):
            ref = tsr.scene_ref(name, 0, 1, seed, **ref_kw(score))
            same(to_host(got, k), ref, "%s, seed %d" % (score, seed))
        assert not np.array_equal(tsr.scene_ref(name, 0, 1, SEEDS[0], **ref_kw(score))["ids"], base["ids"]), score
    got = scored(ctx, tsr.swap_floats(boxes, 4, 6), counts, max_age, 1, tcap, 0, score_at=4)
    for k, seed in enumerate(SEEDS):
        g, ref = to_host(got, k), tsr.scene_ref(name, 0, 1, seed)
        for key in ("ids", "gaps", "hits", "track_info", "track_counts"):
            assert np.array_equal(g[key], ref[key]), key


# ------------------------------------------------------------------ 5. streams
def chunked(ctx, boxes, counts, chunks, slots, max_age, min_hits, tcap, match, assign_at=(), match_at=None, motion_at=()):
    """the clips as streams through `slots`: chunks in assign_at go through dt_associate_stream_tracks_assign, keys of match_at through
    dt_associate_stream_tracks_match, chunks in motion_at through dt_associate_stream_motion, the others through the scored entry
    -> one joined result per clip"""
    match_at = dict(match_at or {})
    n = boxes.shape[0]
    parts, t0 = [[] for _ in range(n)], 0
    for k, L in enumerate(chunks):
        b, c = dev(boxes[:, t0:t0 + L], ctx), dev(counts[:, t0:t0 + L], ctx)
        if k in motion_at:
            i, nid, g = ctx.associate_stream(b, c, THR, slots, max_age=max_age, want_gaps=True, motion_gain=GAIN)
            for q in range(n):
                parts[q].append(blank(i[q].cpu().numpy(), int(nid[q]), g[q].cpu().numpy(), tcap))
            t0 += L
            continue
        if k in match_at:
            r = ctx.associate_stream_tracks(b, c, THR, slots, max_age, GAIN, min_hits, match=match_at[k])
        elif k in assign_at:
            r = ctx.associate_stream_tracks(b, c, THR, slots, max_age, GAIN, min_hits, match=match, assign=True)
        else:
            r = ctx.associate_stream_tracks_scored(b, c, THR, slots, max_age, GAIN, min_hits, tsr.SCORE_HIGH, score_new=tsr.SCORE_NEW,
                                                   assoc_threshold_low=tsr.THR_LOW, max_age_low=tsr.MAX_AGE_LOW, score_at=tsr.SCORE_AT, match=match)
        for q in range(n):
            parts[q].append(to_host(r, q))
        t0 += L
    assert t0 == boxes.shape[1]
    return [join(p) for p in parts]


@pytest.mark.parametrize("name", SCENES)
def test_stream_chunk_invariance(name):
    boxes, counts, tcap, max_age = clips(name)
    match = tsr.SCENES[name][6]
    ctx = ctx_()
    ctx.stream_open(4, boxes.shape[2], track_cap=tcap)
    whole = scored(ctx, boxes, counts, max_age, 2, tcap, match)
    got = chunked(ctx, boxes, counts, CHUNKS[name], [3, 0, 2], max_age, 2, tcap, match)
    for k, seed in enumerate(SEEDS):
        same(got[k], to_host(whole, k), "%s, chunks %s, seed %d: the stateless call" % (name, CHUNKS[name], seed))
        same(got[k], tsr.scene_ref(name, match, 2, seed), "%s, chunks %s, seed %d" % (name, CHUNKS[name], seed))


@pytest.mark.parametrize("other", ["assign", "best_first", "motion"])
@pytest.mark.parametrize("name", ["crowd_reg", "crowd_lds"])
def test_slot_shared_with_the_other_entries(name, other):
    """scored, another entry, scored on one slot.  The other entry finds the dead rows the scored call left for its last frame's
    dropped boxes and must match none of them (the general form's plain assignment is the one whose weights had no such test)."""
    boxes, counts, tcap, max_age = clips(name)
    T, cap = boxes.shape[1:3]
    q = T // 3
    chunks = [q, q, T - 2 * q]
    kw = dict(assign=dict(assign_at=(1,)), best_first=dict(match_at={1: BEST}), motion=dict(motion_at=(1,)))[other]
    ctx = ctx_()
    ctx.stream_open(3, cap, track_cap=tcap)
    got = chunked(ctx, boxes, counts, chunks, [0, 1, 2], max_age, 2, tcap, 0, **kw)
    for k, seed in enumerate(SEEDS):
        b, c = tsr.scene(name, seed)
        ref = tsr.associate_tracks_scored_chunked(b, c, THR, max_age, GAIN, 2, 0, tcap, chunks, **kw)
        assert ref["stats"]["dead_candidates"] > 0 and ref["stats"]["dropped_boxes"] > 0
        assert not np.array_equal(ref["ids"], tsr.scene_ref(name, 0, 2, seed)["ids"]), "vacuous: the mixed run is the scored one"
        same(got[k], ref, "%s: scored, %s, scored; seed %d" % (name, other, seed))


# ------------------------------------------------------------------ 6. refusals
def raw_scored(ctx, b, c, tcap, slots=None, none=(), **over):
    """the two C entries on sentinel-filled outputs -> (return code, the message, the outputs)"""
    import mi355_dt
    n, T, cap, _ = b.shape
    a = dict(thr=THR, max_age=2, tcap=tcap, gain=GAIN, min_hits=2, match=ANY, score_at=6, score_high=0.5, score_new=0.6, thr_low=THR, max_age_low=0)
    a.update(over)
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=ctx.device)
    o = dict(ids=i32(n, T, cap), nids=i32(n), gaps=i32(n, T, cap), hits=i32(n, T, cap), tracks=torch.full((n, T, max(a["tcap"], 1), 8), -7.0, device=ctx.device),
             track_info=i32(n, T, max(a["tcap"], 1), 4), track_counts=i32(n, T))
    p = lambda k: None if k in none else mi355_dt._dptr(o[k])
    ctx._sync_stream()
    outs = (p("ids"), p("nids"), p("gaps"), p("hits"), p("tracks"), p("track_info"), p("track_counts"))
    if slots is None:
        rc = ctx.lib.dt_associate_tracks_scored(ctx.h, mi355_dt._dptr(b), mi355_dt._dptr(c), n, T, cap, a["thr"], a["max_age"], a["tcap"], a["gain"],
                                                a["min_hits"], a["match"], a["score_at"], a["score_high"], a["score_new"], a["thr_low"],
                                                a["max_age_low"], *outs)
    else:
        ns, arr = ctx._slot_array(slots)
        rc = ctx.lib.dt_associate_stream_tracks_scored(ctx.h, mi355_dt._dptr(b), mi355_dt._dptr(c), n, T, cap, a["thr"], a["max_age"], a["gain"],
                                                       a["min_hits"], a["match"], a["score_at"], a["score_high"], a["score_new"], a["thr_low"],
                                                       a["max_age_low"], arr, *outs)
    torch.cuda.synchronize()
    return rc, (ctx.lib.dt_last_error(ctx.h) or b"").decode() if rc else "", o


def untouched(o):
    return all(int((v != -7).sum()) == 0 for v in o.values())


NAN = float("nan")
BAD = (dict(match=1), dict(match=3), dict(match=4), dict(match=8), dict(match=-1), dict(min_hits=0), dict(gain=1.5), dict(gain=NAN), dict(max_age=-1),
       dict(score_at=-1), dict(score_at=8), dict(score_high=NAN), dict(score_new=NAN), dict(thr_low=NAN), dict(max_age_low=-2))
PARTIAL = (("tracks",), ("track_info",), ("track_counts",), ("tracks", "track_info"), ("track_info", "track_counts"), ("tracks", "track_counts"))


def lds_bound(cap):
    """the largest tcap of the general form: 26 * tcap + 5 * cap + 6 words must not exceed 40960 (include/mi355_dt.h)"""
    return (40960 - 6 - 5 * cap) // 26


def test_refusals_leave_outputs_and_slots_unchanged():
    name = "crowd_reg"
    boxes, counts, tcap, max_age = clips(name)
    T, cap = boxes.shape[1:3]
    ctx = ctx_()
    b = lambda a, z: dev(boxes[:1, a:z], ctx)
    c = lambda a, z: dev(counts[:1, a:z], ctx)
    ref = tsr.scene_ref(name, ANY, 2, SEEDS[0])

    # the stateless entry
    for bad in BAD:
        rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), tcap, **bad)
        assert rc == ARG and msg and untouched(o), (bad, rc, msg)
    rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), cap - 1)
    assert rc == ARG and msg and untouched(o)
    for none in PARTIAL + (("ids",), ("nids",)):
        rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), tcap, none=none)
        assert rc == ARG and msg and untouched(o), none
    rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), tcap, none=("gaps", "hits", "tracks", "track_info", "track_counts"))
    assert rc == 0 and np.array_equal(o["ids"][0].cpu().numpy(), ref["ids"][:4]) and untouched({k: o[k] for k in ("gaps", "hits", "tracks")})
    # the LDS bound of the header: the bound itself runs, one entry more is refused and nothing is launched
    top = lds_bound(cap)
    assert 26 * top + 5 * cap + 6 <= 40960 < 26 * (top + 1) + 5 * cap + 6
    rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), top, none=("tracks", "track_info", "track_counts"))
    assert rc == 0, msg
    for key in ("ids", "gaps", "hits"):
        assert np.array_equal(o[key][0].cpu().numpy(), ref[key][:4]), key
    rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), top + 1, none=("tracks", "track_info", "track_counts"))
    assert rc == ARG and "LDS" in msg and untouched(o)
    ctx.stream_open(1, cap, track_cap=top + 1)
    rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), top + 1, slots=[0], none=("tracks", "track_info", "track_counts"))
    assert rc == ARG and "LDS" in msg and untouched(o)
    ctx.stream_open(1, cap, track_cap=top)
    rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), top, slots=[0], none=("tracks", "track_info", "track_counts"))
    assert rc == 0 and np.array_equal(o["ids"][0].cpu().numpy(), ref["ids"][:4]), msg
    # the register form keeps the assignment's 260 * cap + 512 bytes whatever the scores need
    rc, msg, o = raw_scored(ctx, b(0, 4), c(0, 4), 64)
    assert rc == 0, msg

    # the stream entry: refused calls between two valid ones
    ctx.stream_open(4, cap, track_cap=tcap)
    rc, msg, o1 = raw_scored(ctx, b(0, 5), c(0, 5), tcap, slots=[2])
    assert rc == 0, msg
    for bad in BAD:
        rc, msg, o = raw_scored(ctx, b(5, T), c(5, T), tcap, slots=[2], **bad)
        assert rc == ARG and msg and untouched(o), (bad, rc, msg)
    for slots in ([4], [-1]):
        rc, msg, o = raw_scored(ctx, b(5, T), c(5, T), tcap, slots=slots)
        assert rc == ARG and msg and untouched(o), slots
    for none in PARTIAL:
        rc, msg, o = raw_scored(ctx, b(5, T), c(5, T), tcap, slots=[2], none=none)
        assert rc == ARG and msg and untouched(o), none
    rc, msg, o = raw_scored(ctx, dev(boxes[:1, 5:T, :cap - 1], ctx), c(5, T), tcap, slots=[2])      # cap differs from the table's
    assert rc == ARG and msg and untouched(o)
    rc, msg, o2 = raw_scored(ctx, b(5, T), c(5, T), tcap, slots=[2])
    assert rc == 0, msg
    got = join([{k: (int(o[k][0]) if k == "nids" else o[k][0].cpu().numpy()) for k in tsr.KEYS} for o in (o1, o2)])
    same(got, ref, "after the refused calls")
    alone = tsr.associate_tracks_scored(boxes[0, 5:], counts[0, 5:], THR, max_age, GAIN, 2, ANY, tcap)
    assert not np.array_equal(ref["hits"][5:], alone["hits"]), "vacuous: the second chunk does not depend on the slot"


# ------------------------------------------------------------------ 7. the library exports the entries
def test_library_exports_the_scored_entries():
    import subprocess
    import mi355_dt
    out = subprocess.run(["nm", "-D", "--defined-only", mi355_dt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("dt_associate_tracks_scored", "dt_associate_stream_tracks_scored"):
        assert name in exported and name in mi355_dt.SYMBOLS
    assert ctx_().lib.dt_abi_version() == 108      # additions only


# ------------------------------------------------------------------ 8. the tracker class
def test_tracker_with_score_high():
    from test_gpu_stream import small_frames, small_tracker as boxed_tracker      # (its head is scaled so that the frames carry boxes)
    import mi355_dt
    trk = boxed_tracker()[0]
    ctx = trk.model.ctx
    assert trk.SCORE_HIGH is None and trk.SCORE_NEW is None and trk.ASSOC_THRESHOLD_LOW is None and trk.MAX_AGE_LOW == 0 and trk.SCORE_AT == 6
    frames = torch.from_numpy(small_frames(2, 9, seed0=360))
    before = trk.track_clips(frames)
    assert set(before) == {"boxes", "counts", "ids", "nids", "netout"}
    low = trk.OBJ_THRESHOLD * 0.5
    trk.OBJ_THRESHOLD = low      # on the instance: the class and the other tests' tracker stay as they are
    try:
        wide = trk.track_clips(frames)
        score = wide["boxes"][..., 6][wide["ids"] >= 0]
        assert score.numel() > 8
        high = float(score.median())      # half of the boxes weak
        trk.SCORE_HIGH, trk.MAX_AGE, trk.MOTION_GAIN = high, 1, 0.5
        ctx.profile_reset(); ctx.profile_enable(True)
        r = trk.track_clips(frames)
        ctx.profile_enable(False)
        assert "associate:tracks_scored" in ctx.profile_names()
        assert {"ids", "nids", "gaps", "hits"} <= set(r) and "tracks" not in r
        assert torch.equal(r["boxes"].view(torch.int32), wide["boxes"].view(torch.int32)) and torch.equal(r["counts"], wide["counts"])
        want = ctx.associate_tracks_scored(r["boxes"], r["counts"], trk.ASSOC_THRESHOLD, 1, 0.5, 1, high, track_cap=trk.TRACK_CAP, readout=False)
        for key in ("ids", "nids", "gaps", "hits"):
            assert torch.equal(r[key], want[key]), key
        used = torch.arange(r["ids"].shape[2], device=r["ids"].device)[None, None, :] < r["counts"][..., None]
        print("boxes %d, dropped %d, ids %s (plain: %s)" % (int(used.sum()), int(((r["ids"] < 0) & used).sum()), r["nids"].tolist(), wide["nids"].tolist()))
        assert int(((r["ids"] < 0) & used).sum()) > 0 and int((r["hits"][used & (r["ids"] < 0)] != 0).sum()) == 0
        assert set(trk.empty_result(9)) >= {"gaps", "hits"}
        trk.MIN_HITS = 2
        assert {"tracks", "track_info", "track_counts"} <= set(trk.track_clips(frames))
        del trk.MIN_HITS
        trk.open_streams(3)
        ctx.profile_reset(); ctx.profile_enable(True)
        parts = [trk.track_stream(frames[:, :3], [2, 0]), trk.track_stream(frames[:, 3:], [2, 0])]
        ctx.profile_enable(False)
        assert "associate:stream_tracks_scored" in ctx.profile_names()
        for key in ("ids", "gaps", "hits"):
            assert torch.equal(torch.cat([p[key] for p in parts], dim=1), want[key]), key
        assert torch.equal(parts[-1]["nids"], want["nids"])
        trk.MATCH_BEST_FIRST = True      # an order means nothing to an assignment: the library's refusal surfaces
        with pytest.raises(mi355_dt.NativeError) as e:
            trk.track_clips(frames)
        assert int(re.search(r"failed \((\d+)\)", str(e.value)).group(1)) == ARG
    finally:
        for k in ("OBJ_THRESHOLD", "SCORE_HIGH", "MAX_AGE", "MOTION_GAIN", "MIN_HITS", "MATCH_BEST_FIRST"):
            if k in vars(trk):
                delattr(trk, k)
    after = trk.track_clips(frames)
    for key in ("boxes", "counts", "ids", "nids"):
        assert torch.equal(after[key], before[key]), key
