"""GPU suite (-m gpu): track match policy -- best-IoU-first order and label-free matching.

Everything is compared exactly with the plain restatement tests/track_match_ref.py, floats through an int32 view: the IoU keys
are compared as bits in the kernel, decode.hip forms no fused multiply-add, and the rest is the track read-out's.  Both kernel
forms are covered: registers (tcap <= 64 and T <= 64) and LDS (any tcap).
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import track_match_ref as tmr
import track_readout_ref as tro

from test_gpu_track_memory import big_tracker, dev, small_tracker
from test_gpu_track_readout import bits, blank, join, same, to_host

pytestmark = pytest.mark.gpu

THR = 0.3
GAIN = 0.5
BEST, ANY = tmr.MATCH_BEST_FIRST, tmr.MATCH_ANY_LABEL
PARITY_CASES = ("register_form_edge", "lds_form", "longer_than_64_frames", "table_over_64_then_small", "empty_frames")

_REF = {}


def ctx_():
    return small_tracker()[0].model.ctx


def seq(case):
    T, cap, n_obj_t, tcap, chunkings = tmr.CASES[case]
    key = ("seq", case)
    if key not in _REF:
        _REF[key] = tmr.moving_boxes(T, cap, n_obj_t, seed=7)
    return _REF[key] + (tcap, chunkings)


def ref_of(case, match, max_age=3, min_hits=2):
    """the restatement on a CASES entry (seed 7, gain 0.5), computed once per (case, match, max_age); min_hits filters the read-out"""
    key = (case, match, max_age)
    if key not in _REF:
        boxes, counts, tcap, _ = seq(case)
        _REF[key] = tmr.associate_tracks_match(boxes, counts, THR, max_age, GAIN, 1, match, tcap)
    return tro.with_min_hits(_REF[key], min_hits)


def gpu_clip(ctx, boxes, counts, max_age, min_hits, tcap, match, gain=GAIN):
    return to_host(ctx.associate_tracks(dev(boxes[None], ctx), dev(counts[None], ctx), THR, max_age, gain, min_hits, track_cap=tcap,
                                        match=match))


def raw_match(ctx, b, c, max_age, tcap, gain, min_hits, match, gaps=True, hits=True, tracks=True, tinfo=True, tcounts=True, slots=None):
    """the two C entries with any of the optional outputs NULL -> (return code, dict of the outputs given)"""
    import mi355_dt
    n, T, cap, _ = b.shape
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=ctx.device)
    o = dict(ids=i32(n, T, cap), nids=i32(n), gaps=i32(n, T, cap) if gaps else None, hits=i32(n, T, cap) if hits else None,
             tracks=torch.full((n, T, tcap, 8), -7.0, device=ctx.device) if tracks else None,
             track_info=i32(n, T, tcap, 4) if tinfo else None, track_counts=i32(n, T) if tcounts else None)
    p = lambda k: mi355_dt._dptr(o[k])
    ctx._sync_stream()
    if slots is None:
        rc = ctx.lib.dt_associate_tracks_match(ctx.h, mi355_dt._dptr(b), mi355_dt._dptr(c), n, T, cap, THR, max_age, tcap, gain, min_hits,
                                               match, p("ids"), p("nids"), p("gaps"), p("hits"), p("tracks"), p("track_info"),
                                               p("track_counts"))
    else:
        ns, arr = ctx._slot_array(slots)
        rc = ctx.lib.dt_associate_stream_tracks_match(ctx.h, mi355_dt._dptr(b), mi355_dt._dptr(c), n, T, cap, THR, max_age, gain, min_hits,
                                                      match, arr, p("ids"), p("nids"), p("gaps"), p("hits"), p("tracks"), p("track_info"),
                                                      p("track_counts"))
    torch.cuda.synchronize()
    return rc, o


def equal_outputs(o, full, what):
    for k, v in o.items():
        if v is not None:
            g, w = (v.view(torch.int32), full[k].view(torch.int32)) if k == "tracks" else (v, full[k])
            assert torch.equal(g, w), (what, k)


def gpu_chunked(ctx, boxes, counts, chunks, slot, max_age, min_hits, tcap, match, motion_at=()):
    """one stream through slot `slot`; match an int or one per chunk; chunks in motion_at go through dt_associate_stream_motion"""
    ms = [match] * len(chunks) if np.isscalar(match) else list(match)
    parts, t0 = [], 0
    for k, L in enumerate(chunks):
        b, c = dev(boxes[None, t0:t0 + L], ctx), dev(counts[None, t0:t0 + L], ctx)
        if k in motion_at:
            i, nid, g = ctx.associate_stream(b, c, THR, [slot], max_age=max_age, want_gaps=True, motion_gain=GAIN)
            parts.append(blank(i[0].cpu().numpy(), int(nid[0]), g[0].cpu().numpy(), tcap))
        else:
            parts.append(to_host(ctx.associate_stream_tracks(b, c, THR, [slot], max_age, GAIN, min_hits, match=ms[k])))
        t0 += L
    assert t0 == boxes.shape[0]
    return join(parts)


# ------------------------------------------------------------------ 1. parity of all seven outputs with the restatement
@pytest.mark.parametrize("match", [BEST, ANY, BEST | ANY])
@pytest.mark.parametrize("case", PARITY_CASES)
def test_parity_with_restatement(case, match):
    boxes, counts, tcap, _ = seq(case)
    T = boxes.shape[0]
    ctx = ctx_()
    register_form = case in ("register_form_edge", "empty_frames")
    assert register_form == (tcap <= 64 and T <= 64)      # which form the launcher takes, from tcap and T alone
    ref = ref_of(case, match)
    if match & ANY or case in ("register_form_edge", "lds_form"):      # (in the sparser scenes best-first finds today's pairs)
        assert not np.array_equal(ref["ids"], ref_of(case, 0)["ids"]), "vacuous: match %d finds today's ids" % match
    same(gpu_clip(ctx, boxes, counts, 3, 2, tcap, match), ref, "%s, match %d" % (case, match))
    if boxes.shape[1] <= 64:                                           # (the dense scenes' restatement takes seconds per run)
        same(gpu_clip(ctx, boxes, counts, 0, 1, tcap, match), ref_of(case, match, 0, 1), "%s, match %d, max_age 0" % (case, match))


def test_worked_example():
    """DESIGN.md's two frames in both forms: today's order opens a third id, best-first keeps two"""
    ctx = ctx_()
    boxes = np.zeros((2, 2, 8), dtype=np.float32)
    for t, xs in enumerate(((0.30, 0.40), (0.36, 0.43))):
        for i, x in enumerate(xs):
            boxes[t, i] = [x, 0.5, 0.2, 0.2, 0.9, 0, 0.8, i]
    counts = np.array([2, 2], dtype=np.int32)
    for tcap in (2, 80):
        for any_label in (0, ANY):
            today = gpu_clip(ctx, boxes, counts, 0, 1, tcap, any_label, gain=0.0)
            best = gpu_clip(ctx, boxes, counts, 0, 1, tcap, BEST | any_label, gain=0.0)
            assert today["ids"].tolist() == [[0, 1], [1, 2]] and today["nids"] == 3, tcap
            assert best["ids"].tolist() == [[0, 1], [0, 1]] and best["nids"] == 2, tcap
            same(best, tmr.associate_tracks_match(boxes, counts, THR, 0, 0.0, 1, BEST | any_label, tcap), "tcap %d" % tcap)


# ------------------------------------------------------------------ 2. match = 0 is the existing entry
@pytest.mark.parametrize("case", ["register_form_edge", "lds_form", "longer_than_64_frames"])
def test_match_0_is_dt_associate_tracks(case):
    boxes, counts, tcap, _ = seq(case)
    ctx = ctx_()
    b, c = dev(boxes[None], ctx), dev(counts[None], ctx)
    for a, g, m in ((3, GAIN, 2), (0, 1.0, 1)):
        full = ctx.associate_tracks(b, c, THR, a, g, m, track_cap=tcap)
        rc, o = raw_match(ctx, b, c, a, tcap, g, m, 0)
        assert rc == 0
        equal_outputs(o, full, (a, g, m))
    # ... and in a stream
    ctx.stream_open(2, boxes.shape[1], track_cap=tcap)
    L = boxes.shape[0] // 2
    for t0, t1 in ((0, L), (L, boxes.shape[0])):
        want = ctx.associate_stream_tracks(b[:, t0:t1].contiguous(), c[:, t0:t1].contiguous(), THR, [0], 3, GAIN, 2)
        rc, o = raw_match(ctx, b[:, t0:t1].contiguous(), c[:, t0:t1].contiguous(), 3, tcap, GAIN, 2, 0, slots=[1])
        assert rc == 0
        equal_outputs(o, want, (t0, t1))


# ------------------------------------------------------------------ 3. optional outputs NULL
@pytest.mark.parametrize("case", ["register_form_edge", "lds_form"])
def test_optional_outputs_null(case):
    boxes, counts, tcap, _ = seq(case)
    ctx = ctx_()
    b, c = dev(boxes[None], ctx), dev(counts[None], ctx)
    full = ctx.associate_tracks(b, c, THR, 3, GAIN, 2, track_cap=tcap, match=BEST | ANY)
    for off in (dict(gaps=False), dict(hits=False), dict(gaps=False, hits=False), dict(tracks=False, tinfo=False, tcounts=False),
                dict(gaps=False, hits=False, tracks=False, tinfo=False, tcounts=False)):
        rc, o = raw_match(ctx, b, c, 3, tcap, GAIN, 2, BEST | ANY, **off)
        assert rc == 0, off
        equal_outputs(o, full, off)
    lean = ctx.associate_tracks(b, c, THR, 3, GAIN, 2, track_cap=tcap, match=BEST | ANY, readout=False)
    assert set(lean) == {"ids", "nids", "gaps", "hits"}
    equal_outputs(lean, full, "readout=False")


# ------------------------------------------------------------------ 4. many clips in one call
@pytest.mark.parametrize("tcap", [64, 80])
def test_48_clips_in_one_call(tcap):
    """one wavefront per clip: 48 clips of different seeds in one launch, in the register form (tcap 64) and in the LDS form
    (tcap 80; no entry is cut in either, so one match serves both -- the read-out is laid out again for the wider rows)"""
    ctx = ctx_()
    T, cap = 10, 32
    if "clips48" not in _REF:
        seqs = [tmr.moving_boxes(T, cap, (lambda t, k=k: 6 + k % 7), seed=100 + k) for k in range(48)]
        refs = [tmr.associate_tracks_match(b, c, THR, 3, GAIN, 2, BEST | ANY, 64) for b, c in seqs]
        assert all(r["dropped"] == 0 for r in refs)
        _REF["clips48"] = (seqs, refs)
    seqs, refs = _REF["clips48"]
    b = np.stack([s[0] for s in seqs]); c = np.stack([s[1] for s in seqs])
    got = ctx.associate_tracks(dev(b, ctx), dev(c, ctx), THR, 3, GAIN, 2, track_cap=tcap, match=BEST | ANY)
    for k in range(48):
        ref = dict(refs[k])
        ref.update(tro.read_out(refs[k]["table"], 2, tcap))
        same(to_host(got, k), ref, "clip %d" % k)


# ------------------------------------------------------------------ 5. the capacity cut
def test_capacity_cut_lds_form():
    """CASES' own table: 120 then 20 objects with max_age 8 overflow the 160 entries under the best-first order"""
    ctx = ctx_()
    boxes, counts, tcap, _ = seq("table_over_64_then_small")
    for match in (BEST, ANY):
        tight = ref_of("table_over_64_then_small", match, 8, 2)
        print("match %d: tcap %d cuts %d entries" % (match, tcap, tight["dropped"]))
        if match == BEST:
            assert tight["dropped"] > 0
            assert max(len(rows) for rows in tight["table"]) == tcap, "the table is never full"
        same(gpu_clip(ctx, boxes, counts, 8, 2, tcap, match), tight, "match %d, tcap %d" % (match, tcap))


def test_capacity_cut_register_form():
    """the read-out suite's register shape: 30 objects in frames of at most 32 boxes, a table of 36 entries -- the cut inside the
    register form's lane permutation behind a best-first match"""
    ctx = ctx_()
    T, cap, tcap = 40, 32, 36
    boxes, counts = tmr.moving_boxes(T, cap, lambda t: 30, seed=7)
    for match in (BEST, BEST | ANY):
        tight = tmr.associate_tracks_match(boxes, counts, THR, 8, GAIN, 2, match, tcap)
        assert tight["dropped"] > 0 and max(len(rows) for rows in tight["table"]) == tcap
        same(gpu_clip(ctx, boxes, counts, 8, 2, tcap, match), tight, "match %d, tcap %d" % (match, tcap))


# ------------------------------------------------------------------ 6. best-first does not depend on the order of a frame's boxes
@pytest.mark.parametrize("any_label", [0, ANY])
@pytest.mark.parametrize("scene", sorted(tmr.PERMUTATION_SCENES))
def test_permutation_invariance(scene, any_label):
    ctx = ctx_()
    T, cap, n_obj, tcap = tmr.PERMUTATION_SCENES[scene]
    assert (scene == "register_form") == (tcap <= 64 and T <= 64)
    boxes, counts, _ = tmr.moving_boxes_gt(T, cap, lambda t: n_obj, seed=7, duplicates=False)
    shuffled = tmr.permute_frames(boxes, counts, seed=11)
    match = BEST | any_label
    parts = []
    for bx in (boxes, shuffled):
        ref = tmr.associate_tracks_match(bx, counts, THR, 3, GAIN, 1, match, tcap)
        assert ref["ties"] == 0 and ref["dropped"] == 0 and counts.min() >= 2      # the property's three preconditions
        got = gpu_clip(ctx, bx, counts, 3, 1, tcap, match)
        same(got, ref, scene)
        parts.append(tmr.partition(got["ids"], bx, counts))
    assert parts[0] == parts[1], "the tracks depend on the order of the boxes"
    if scene == "general_form_dense" and not any_label:
        a, b = (gpu_clip(ctx, bx, counts, 3, 1, tcap, 0) for bx in (boxes, shuffled))
        assert tmr.partition(a["ids"], boxes, counts) != tmr.partition(b["ids"], shuffled, counts), "vacuous: today's order is invariant here"


# ------------------------------------------------------------------ 7. streams
@pytest.mark.parametrize("case", PARITY_CASES)
def test_stream_chunk_invariance(case):
    boxes, counts, tcap, chunkings = seq(case)
    ctx = ctx_()
    ctx.stream_open(2, boxes.shape[1], track_cap=tcap)
    for match in (BEST, BEST | ANY):
        ref = ref_of(case, match)
        whole = gpu_clip(ctx, boxes, counts, 3, 2, tcap, match)
        for chunks in chunkings:
            ctx.stream_reset([1])
            got = gpu_chunked(ctx, boxes, counts, chunks, 1, 3, 2, tcap, match)
            same(got, whole, "%s, match %d, chunks %s against the stateless call" % (case, match, chunks))
            same(got, ref, "%s, match %d, chunks %s" % (case, match, chunks))


@pytest.mark.parametrize("case", ["register_form_edge", "table_over_64_then_small"])
def test_chunks_with_different_policies_on_one_slot(case):
    boxes, counts, tcap, _ = seq(case)
    T, cap = boxes.shape[:2]
    ctx = ctx_()
    q = T // 4
    chunks, ms = [q, q, q, T - 3 * q], [0, BEST | ANY, BEST, ANY]
    ref = tmr.associate_tracks_match_chunked(boxes, counts, THR, 3, GAIN, 2, ms, tcap, chunks)
    for m in range(4):
        assert not np.array_equal(ref["ids"], ref_of(case, m)["ids"]), "vacuous: the mixed run is match %d's" % m
    ctx.stream_open(2, cap, track_cap=tcap)
    same(gpu_chunked(ctx, boxes, counts, chunks, 1, 3, 2, tcap, ms), ref, "policies %s over chunks %s" % (ms, chunks))


@pytest.mark.parametrize("case", ["register_form_edge", "table_over_64_then_small"])
def test_slot_shared_with_the_motion_entry(case):
    """dt_associate_stream_motion, a match-policy call, dt_associate_stream_motion, a match-policy call on one slot: the table,
    its velocities and ids carry over both ways; the hits are forgotten by the motion entry, as for the read-out entry"""
    boxes, counts, tcap, _ = seq(case)
    T, cap = boxes.shape[:2]
    ctx = ctx_()
    q = T // 4
    chunks = [q, q, q, T - 3 * q]
    ref = tmr.associate_tracks_match_chunked(boxes, counts, THR, 3, GAIN, 2, BEST | ANY, tcap, chunks, motion_at=(0, 2))
    unmixed = ref_of(case, BEST | ANY)
    assert not np.array_equal(ref["ids"], unmixed["ids"])
    ctx.stream_open(1, cap, track_cap=tcap)
    same(gpu_chunked(ctx, boxes, counts, chunks, 0, 3, 2, tcap, BEST | ANY, motion_at=(0, 2)), ref, "motion, match, motion, match")


def test_reset():
    ctx = ctx_()
    case = "register_form_edge"
    boxes, counts, tcap, _ = seq(case)
    T, cap = boxes.shape[:2]
    ref = ref_of(case, BEST | ANY)
    head = tmr.associate_tracks_match(boxes[:12], counts[:12], THR, 3, GAIN, 2, BEST | ANY, tcap)
    ctx.stream_open(3, cap, track_cap=tcap)
    first = gpu_chunked(ctx, boxes[:12], counts[:12], [12], 2, 3, 2, tcap, BEST | ANY)
    other = gpu_chunked(ctx, boxes[:12], counts[:12], [12], 0, 3, 2, tcap, BEST | ANY)
    same(first, head, "fresh slot")
    ctx.stream_reset([2])
    again = gpu_chunked(ctx, boxes[:12], counts[:12], [5, 7], 2, 3, 2, tcap, BEST | ANY)
    same(again, head, "the reset slot starts over")
    rest = gpu_chunked(ctx, boxes[12:], counts[12:], [T - 12], 0, 3, 2, tcap, BEST | ANY)
    same(join([other, rest]), ref, "neighbour of a reset slot")
    rest = gpu_chunked(ctx, boxes[12:], counts[12:], [T - 12], 2, 3, 2, tcap, BEST | ANY)
    same(join([again, rest]), ref, "the reset slot, continued")


# ------------------------------------------------------------------ 8. errors
def _code(excinfo):
    return int(re.search(r"failed \((\d+)\)", str(excinfo.value)).group(1))


def test_errors_leave_the_state_unchanged():
    import mi355_dt
    trk, blob, tw = small_tracker()
    ctx = trk.model.ctx
    ARG, STATE = 1, 3
    M = BEST | ANY
    T, cap, tcap = 20, 32, 64
    boxes, counts = tmr.moving_boxes(T, cap, lambda t: 12, seed=7)
    ref = tmr.associate_tracks_match(boxes, counts, THR, 3, GAIN, 2, M, tcap)
    b = lambda a, z: dev(boxes[None, a:z], ctx)
    c = lambda a, z: dev(counts[None, a:z], ctx)
    partial = (dict(tracks=False), dict(tinfo=False), dict(tcounts=False), dict(tracks=False, tinfo=False), dict(tinfo=False, tcounts=False),
               dict(tracks=False, tcounts=False))

    fresh = type(trk)(detector_weights=blob, tracker_weights=tw)      # no stream_open yet
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.model.ctx.associate_stream_tracks(b(0, 4), c(0, 4), THR, [0], 3, GAIN, 2, match=M)
    assert _code(e) == STATE
    fresh.model.ctx.close()

    # the stateless entry
    for bad in (dict(match=-1), dict(match=4), dict(match=8), dict(min_hits=0), dict(gain=1.5), dict(gain=float("nan")), dict(max_age=-1),
                dict(track_cap=31)):
        kw = dict(max_age=3, gain=GAIN, min_hits=2, track_cap=tcap, match=M)
        kw.update(bad)
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_tracks(b(0, 4), c(0, 4), THR, kw["max_age"], kw["gain"], kw["min_hits"], track_cap=kw["track_cap"], match=kw["match"])
        assert _code(e) == ARG, bad
    for off in partial:
        assert raw_match(ctx, b(0, 4), c(0, 4), 3, tcap, GAIN, 2, M, **off)[0] == ARG, off
    # cap 128, 2040 entries: 20 * 2040 + 128 words fit the LDS, the best-first order's 20 * 2040 + 4 * 128 do not -- refused, never launched
    wide, wcounts, _, _ = seq("lds_form")
    wb = lambda a, z: dev(wide[None, a:z], ctx)
    wc = lambda a, z: dev(wcounts[None, a:z], ctx)
    ctx.associate_tracks(wb(0, 2), wc(0, 2), THR, 3, GAIN, 2, track_cap=2040, match=ANY)
    for m in (BEST, M):
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_tracks(wb(0, 2), wc(0, 2), THR, 3, GAIN, 2, track_cap=2040, match=m)
        assert _code(e) == ARG
    ctx.stream_open(2, 128, track_cap=2040)
    r1 = to_host(ctx.associate_stream_tracks(wb(0, 4), wc(0, 4), THR, [0], 3, GAIN, 2, match=ANY))
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_stream_tracks(wb(4, 8), wc(4, 8), THR, [0], 3, GAIN, 2, match=M)
    assert _code(e) == ARG
    r2 = to_host(ctx.associate_stream_tracks(wb(4, 8), wc(4, 8), THR, [0], 3, GAIN, 2, match=ANY))
    want = ref_of("lds_form", ANY)
    for key in ("ids", "gaps", "hits"):
        assert np.array_equal(np.concatenate([r1[key], r2[key]]), want[key]), key
    assert r2["nids"] == want["nids"]

    # the stream entry: refused calls between two valid ones
    ctx.stream_open(4, cap, track_cap=tcap)
    r1 = to_host(ctx.associate_stream_tracks(b(0, 9), c(0, 9), THR, [2], 3, GAIN, 2, match=M))
    for bad in (dict(match=-1), dict(match=4), dict(min_hits=0), dict(gain=1.5), dict(gain=float("nan")), dict(max_age=-1), dict(slots=[4]),
                dict(slots=[-1])):
        kw = dict(max_age=3, gain=GAIN, min_hits=2, slots=[2], match=M)
        kw.update(bad)
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_stream_tracks(b(9, 20), c(9, 20), THR, kw["slots"], kw["max_age"], kw["gain"], kw["min_hits"], match=kw["match"])
        assert _code(e) == ARG, bad
    for off in partial:
        assert raw_match(ctx, b(9, 20), c(9, 20), 3, tcap, GAIN, 2, M, slots=[2], **off)[0] == ARG, off
    with pytest.raises(mi355_dt.NativeError) as e:      # a slot named twice
        ctx.associate_stream_tracks(dev(boxes[None, 9:11].repeat(2, 0), ctx), dev(counts[None, 9:11].repeat(2, 0), ctx), THR, [2, 2], 3, GAIN, 2,
                                    match=M)
    assert _code(e) == ARG
    with pytest.raises(mi355_dt.NativeError) as e:      # cap differs from the table's
        ctx.associate_stream_tracks(dev(boxes[None, 9:20, :31], ctx), c(9, 20), THR, [2], 3, GAIN, 2, match=M)
    assert _code(e) == ARG
    n, arr = ctx._slot_array([2])
    assert ctx.lib.dt_associate_stream_tracks_match(ctx.h, None, None, 1, 3, cap, 0.3, 3, 0.5, 2, M, arr, None, None, None, None, None, None,
                                                    None) == ARG
    assert ctx.lib.dt_associate_tracks_match(ctx.h, None, None, 1, 3, cap, 0.3, 3, tcap, 0.5, 2, M, None, None, None, None, None, None, None) == ARG
    r2 = to_host(ctx.associate_stream_tracks(b(9, 20), c(9, 20), THR, [2], 3, GAIN, 2, match=M))
    same(join([r1, r2]), ref, "after the refused calls")
    alone = tmr.associate_tracks_match(boxes[9:], counts[9:], THR, 3, GAIN, 2, M, tcap)
    assert not np.array_equal(ref["hits"][9:], alone["hits"]), "vacuous: the second chunk does not depend on the slot"


# ------------------------------------------------------------------ 9. the library exports the entries
def test_library_exports_the_match_entries():
    import mi355_dt
    out = subprocess.run(["nm", "-D", "--defined-only", mi355_dt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("dt_associate_tracks_match", "dt_associate_stream_tracks_match"):
        assert name in exported and name in mi355_dt.SYMBOLS
    header = open(os.path.join(os.path.dirname(mi355_dt.LIB_PATH), "..", "include", "mi355_dt.h")).read()
    assert "dt_associate_tracks_match(" in header and "dt_associate_stream_tracks_match(" in header
    assert (mi355_dt.DT_MATCH_BEST_FIRST, mi355_dt.DT_MATCH_ANY_LABEL) == (BEST, ANY)
    assert ctx_().lib.dt_abi_version() == 108


# ------------------------------------------------------------------ 10. end to end at 416
def test_end_to_end_416():
    from parallel import pinned_policy
    trk, blob, tw, fr = big_tracker()
    assert not trk.MATCH_BEST_FIRST and not trk.MATCH_ANY_LABEL

    class Mot(type(trk)):
        MAX_AGE = 2
        MOTION_GAIN = 0.5
        MATCH_BEST_FIRST = True
        MATCH_ANY_LABEL = True

    mot = Mot(detector_weights=blob, tracker_weights=tw)
    try:
        lean = ("netout", "boxes", "counts", "ids", "gaps", "hits")
        readout = ("tracks", "track_info", "track_counts")
        mot.open_streams(4)
        ctx = mot.model.ctx
        with pinned_policy(ctx):
            ctx.profile_reset(); ctx.profile_enable(True)
            ref = mot.track_clips(fr)
            ctx.profile_enable(False)
            names = ctx.profile_names()
            assert "associate:tracks_match" in names and "associate:tracks" not in names and "associate:motion" not in names
            assert set(ref) == set(lean) | {"nids"}      # MIN_HITS is None: no read-out
            n_clips, T, cap = ref["ids"].shape
            assert (n_clips, T) == (2, 30) and int(ref["counts"].sum()) > 0
            # the Context call on the boxes the GPU decoded, and the restatement on them
            want = ctx.associate_tracks(ref["boxes"], ref["counts"], mot.ASSOC_THRESHOLD, 2, 0.5, 1, match=BEST | ANY)
            for key in ("ids", "nids", "gaps", "hits"):
                assert torch.equal(ref[key], want[key]), key
            for k in range(n_clips):
                b, c = ref["boxes"][k].cpu().numpy(), ref["counts"][k].cpu().numpy()
                same(to_host(want, k), tmr.associate_tracks_match(b, c, mot.ASSOC_THRESHOLD, 2, 0.5, 1, BEST | ANY, cap), "416, clip %d" % k)
            frames = mot.boxes_from_result(ref, 0)
            hits = ref["hits"][0].cpu().numpy()
            assert all([bb.track_hits for bb in frames[t]] == hits[t, :len(frames[t])].tolist() for t in range(T))
            e = mot.empty_result(T)
            assert set(e) == set(lean) | {"nids"}
            # streams in chunks
            ctx.profile_reset(); ctx.profile_enable(True)
            parts, t0 = [], 0
            for L in (7, 23):
                parts.append(mot.track_stream(fr[:, t0:t0 + L], [1, 3]))
                t0 += L
            ctx.profile_enable(False)
            assert "associate:stream_tracks_match" in ctx.profile_names()
            for key in lean:
                got = torch.cat([p[key] for p in parts], dim=1)
                assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                                   ref[key].view(torch.int32) if got.dtype == torch.float32 else ref[key]), key
            assert torch.equal(parts[-1]["nids"], ref["nids"])
            # with MIN_HITS the read-out keys appear, and the match is the same
            mot.MIN_HITS = 2
            full = mot.track_clips(fr)
            assert set(full) == set(lean) | set(readout) | {"nids"}
            want = ctx.associate_tracks(ref["boxes"], ref["counts"], mot.ASSOC_THRESHOLD, 2, 0.5, 2, match=BEST | ANY)
            for key in ("ids", "nids", "gaps", "hits", "track_info", "track_counts"):
                assert torch.equal(full[key], want[key]), key
            assert torch.equal(full["tracks"].view(torch.int32), want["tracks"].view(torch.int32))
            assert torch.equal(full["ids"], ref["ids"]) and int(full["track_counts"].sum()) > 0
    finally:
        mot.model.ctx.close()
