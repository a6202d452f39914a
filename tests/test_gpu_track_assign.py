"""GPU suite (-m gpu): track assignment -- the optimal (maximum summed IoU) one-to-one match of a frame's boxes to the track table
(dt_associate_tracks_assign and its stream entry).

Everything is compared exactly with the plain restatement tests/track_assign_ref.py, floats through an int32 view: the weights are
integers, the solver is exact, and the rest is the track read-out's.  Both kernel forms are covered: registers (tcap <= 64 and
T <= 64) and LDS (any tcap), each with more boxes than entries and with fewer.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import track_assign_ref as tar
import track_match_ref as tmr

from test_gpu_track_memory import dev, small_tracker
from test_gpu_track_readout import blank, join, same, to_host
from test_gpu_track_match import PARITY_CASES, equal_outputs

pytestmark = pytest.mark.gpu

THR, GAIN = tar.THR, tar.GAIN
BEST, ANY = tmr.MATCH_BEST_FIRST, tmr.MATCH_ANY_LABEL
SCENES = sorted(tar.SCENES)
CHUNKINGS = {"crowd_reg_grow": [[1] * 12, [5, 7]], "crowd_reg": [[1] * 12, [4, 1, 7]], "crowd_lds": [[1] * 6, [2, 4]],
             "crowd_long": [[1] * 66, [64, 2], [30, 36]]}
_REF = {}


def ctx_():
    return small_tracker()[0].model.ctx


def setup_of(name):
    """a scene of track_assign_ref or a CASES entry -> (boxes, counts, tcap, max_age)"""
    if name in tar.SCENES:
        return tar.scene(name) + (tar.SCENES[name][3], tar.SCENES[name][4])
    return tar.case_boxes(name) + (tar.CASES[name][3], 3)


def ref_of(name, match, max_age, min_hits, tcap=None):
    boxes, counts, tcap0, _ = setup_of(name)
    return tar.ref(name, boxes, counts, max_age, min_hits, match, tcap0 if tcap is None else tcap)


def gpu_clip(ctx, boxes, counts, max_age, min_hits, tcap, match, gain=GAIN, assign=True):
    return to_host(ctx.associate_tracks(dev(boxes[None], ctx), dev(counts[None], ctx), THR, max_age, gain, min_hits, track_cap=tcap,
                                        match=match, assign=assign))


def raw_assign(ctx, b, c, max_age, tcap, gain, min_hits, match, gaps=True, hits=True, tracks=True, tinfo=True, tcounts=True, slots=None):
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
        rc = ctx.lib.dt_associate_tracks_assign(ctx.h, mi355_dt._dptr(b), mi355_dt._dptr(c), n, T, cap, THR, max_age, tcap, gain, min_hits,
                                                match, p("ids"), p("nids"), p("gaps"), p("hits"), p("tracks"), p("track_info"),
                                                p("track_counts"))
    else:
        ns, arr = ctx._slot_array(slots)
        rc = ctx.lib.dt_associate_stream_tracks_assign(ctx.h, mi355_dt._dptr(b), mi355_dt._dptr(c), n, T, cap, THR, max_age, gain, min_hits,
                                                       match, arr, p("ids"), p("nids"), p("gaps"), p("hits"), p("tracks"), p("track_info"),
                                                       p("track_counts"))
    torch.cuda.synchronize()
    return rc, o


def gpu_chunked(ctx, boxes, counts, chunks, slot, max_age, min_hits, tcap, match, match_at=None, motion_at=()):
    """one stream through slot `slot`: chunks in match_at go through dt_associate_stream_tracks_match with that match, chunks in
    motion_at through dt_associate_stream_motion, the others through dt_associate_stream_tracks_assign with `match`"""
    match_at = dict(match_at or {})
    parts, t0 = [], 0
    for k, L in enumerate(chunks):
        b, c = dev(boxes[None, t0:t0 + L], ctx), dev(counts[None, t0:t0 + L], ctx)
        if k in motion_at:
            i, nid, g = ctx.associate_stream(b, c, THR, [slot], max_age=max_age, want_gaps=True, motion_gain=GAIN)
            parts.append(blank(i[0].cpu().numpy(), int(nid[0]), g[0].cpu().numpy(), tcap))
        elif k in match_at:
            parts.append(to_host(ctx.associate_stream_tracks(b, c, THR, [slot], max_age, GAIN, min_hits, match=match_at[k])))
        else:
            parts.append(to_host(ctx.associate_stream_tracks(b, c, THR, [slot], max_age, GAIN, min_hits, match=match, assign=True)))
        t0 += L
    assert t0 == boxes.shape[0]
    return join(parts)


# ------------------------------------------------------------------ 1. parity of all seven outputs with the restatement
@pytest.mark.parametrize("match", [0, ANY])
@pytest.mark.parametrize("name", SCENES + list(PARITY_CASES))
def test_parity_with_restatement(name, match):
    boxes, counts, tcap, max_age = setup_of(name)
    T, cap = boxes.shape[:2]
    ctx = ctx_()
    register_form = name in ("crowd_reg_grow", "crowd_reg", "register_form_edge", "empty_frames")
    assert register_form == (tcap <= 64 and T <= 64) == (tar.form_of(tcap, T) == "register")      # the form the launcher takes
    ref = ref_of(name, match, max_age, 2)
    got = gpu_clip(ctx, boxes, counts, max_age, 2, tcap, match)
    if name in tar.SCENES and match == tar.SCENES[name][6]:      # (only there is a difference from best-first stated)
        best = gpu_clip(ctx, boxes, counts, max_age, 2, tcap, BEST | match, assign=False)
        assert any(not np.array_equal(ref["ids"][t], best["ids"][t]) for t in range(T)), "vacuous: best-first finds the optimal ids"
        assert any(n > nt > 0 for n, nt, _, _, _ in ref["log"]), "vacuous: the solve is never transposed"
    same(got, ref, "%s, match %d" % (name, match))
    if cap <= 64:
        same(gpu_clip(ctx, boxes, counts, 0, 1, tcap, match), ref_of(name, match, 0, 1), "%s, match %d, max_age 0" % (name, match))


# ------------------------------------------------------------------ 2. the smallest case
def test_worked_example():
    """two boxes compete for one track, in both forms: every greedy policy opens a third id, the assignment keeps both tracks"""
    ctx = ctx_()
    boxes, counts = tar.worked_example()
    for tcap in (2, 80):
        for any_label in (0, ANY):
            for m in (0, BEST):
                old = gpu_clip(ctx, boxes, counts, 0, 1, tcap, m | any_label, gain=0.0, assign=False)
                assert old["ids"].tolist() == [[0, 1], [0, 2]] and old["nids"] == 3, (tcap, m)
            opt = gpu_clip(ctx, boxes, counts, 0, 1, tcap, any_label, gain=0.0)
            assert opt["ids"].tolist() == [[0, 1], [1, 0]] and opt["nids"] == 2, tcap
            same(opt, tar.associate_tracks_assign(boxes, counts, THR, 0, 0.0, 1, any_label, tcap), "tcap %d" % tcap)


# ------------------------------------------------------------------ 3. the pairs are dt_assign_max's
@pytest.mark.parametrize("tcap", [64, 80])
@pytest.mark.parametrize("objects", [(26, 14), (14, 26)], ids=["n_below_nt", "n_above_nt"])
def test_pairs_are_dt_assign_maxs(objects, tcap):
    """two frames, max_age 0, gain 0, any label: frame 0 opens ids 0 .. n0 - 1, the entry indices, so frame 1's ids are row_to_col of
    dt_assign_max on the weights the restatement's candidates give"""
    ctx = ctx_()
    boxes, counts = tar.crowd_boxes(2, 32, lambda t: objects[t], 7, .3)
    n0, n1 = int(counts[0]), int(counts[1])
    assert (n1 < n0) == (objects[1] < objects[0]) and min(n0, n1) >= 8
    tr = tar.TrackAssign(tcap, THR, 0.0, ANY)
    tr.frame(boxes[0, :n0], 0)
    cand = tr.candidates(boxes[1, :n1], 0)
    w = tar.weights(cand, n1, n0).astype(np.int32)
    assert (w > 0).sum() > max(n0, n1), "vacuous: no box has a choice"
    r2c, _, total = ctx.assign_max(dev(w[None], ctx))
    r2c = r2c[0].cpu().numpy()
    got = gpu_clip(ctx, boxes, counts, 0, 1, tcap, ANY, gain=0.0)
    assert got["ids"][0, :n0].tolist() == list(range(n0))
    ids1 = got["ids"][1, :n1]
    assert (r2c >= 0).sum() >= 4 and int(total[0]) == sum(int(w[i, r2c[i]]) for i in range(n1) if r2c[i] >= 0)
    for i in range(n1):
        assert ids1[i] == r2c[i] if r2c[i] >= 0 else ids1[i] >= n0, (i, ids1.tolist(), r2c.tolist())


# ------------------------------------------------------------------ 4. optional outputs NULL
@pytest.mark.parametrize("name", ["crowd_reg_grow", "crowd_lds"])
def test_optional_outputs_null(name):
    boxes, counts, tcap, max_age = setup_of(name)
    ctx = ctx_()
    b, c = dev(boxes[None], ctx), dev(counts[None], ctx)
    full = ctx.associate_tracks(b, c, THR, max_age, GAIN, 2, track_cap=tcap, match=ANY, assign=True)
    for off in (dict(gaps=False), dict(hits=False), dict(tracks=False, tinfo=False, tcounts=False),
                dict(gaps=False, hits=False, tracks=False, tinfo=False, tcounts=False)):
        rc, o = raw_assign(ctx, b, c, max_age, tcap, GAIN, 2, ANY, **off)
        assert rc == 0, off
        equal_outputs(o, full, off)
    lean = ctx.associate_tracks(b, c, THR, max_age, GAIN, 2, track_cap=tcap, match=ANY, readout=False, assign=True)
    assert set(lean) == {"ids", "nids", "gaps", "hits"}
    equal_outputs(lean, full, "readout=False")


# ------------------------------------------------------------------ 5. many clips in one call
@pytest.mark.parametrize("tcap", [64, 80])
def test_48_clips_in_one_call(tcap):
    """one wavefront per clip: 48 different crowds in one launch equal 48 launches of one, in both forms"""
    ctx = ctx_()
    T, cap = 6, 32
    if "clips48" not in _REF:
        _REF["clips48"] = [tar.crowd_boxes(T, cap, (lambda t, k=k: 8 + k % 9 + 2 * t), 100 + k, .35) for k in range(48)]
    seqs = _REF["clips48"]
    b = dev(np.stack([s[0] for s in seqs]), ctx); c = dev(np.stack([s[1] for s in seqs]), ctx)
    got = ctx.associate_tracks(b, c, THR, 2, GAIN, 2, track_cap=tcap, match=0, assign=True)
    opened = set()
    for k in range(48):
        one = ctx.associate_tracks(b[k:k + 1].contiguous(), c[k:k + 1].contiguous(), THR, 2, GAIN, 2, track_cap=tcap, match=0, assign=True)
        same(to_host(got, k), to_host(one), "clip %d" % k)
        opened.add(int(one["nids"][0]))
    assert len(opened) > 8, "vacuous: the clips are alike"
    for k in (0, 47):
        same(to_host(got, k), tar.associate_tracks_assign(seqs[k][0], seqs[k][1], THR, 2, GAIN, 2, 0, tcap), "clip %d, restatement" % k)


# ------------------------------------------------------------------ 6. the capacity cut
@pytest.mark.parametrize("name,frames,form", [("crowd_long", 60, "register"), ("crowd_lds", 6, "general")])
def test_capacity_cut(name, frames, form):
    """the scenes' tables never outgrow their cap, and tcap may not be below cap: so the boxes are repacked to the largest frame's
    count and the table lowered to it, where the lost tracks no longer all fit (crowd_long: its first 60 frames, the register form)"""
    boxes, counts, _, max_age = setup_of(name)
    tcap = int(counts[:frames].max())
    boxes, counts = np.ascontiguousarray(boxes[:frames, :tcap]), counts[:frames]
    assert tar.form_of(tcap, frames) == form
    ctx = ctx_()
    for match in (0, ANY):
        tight = tar.associate_tracks_assign(boxes, counts, THR, max_age, GAIN, 2, match, tcap)
        print("%s, match %d: tcap %d cuts %d entries" % (name, match, tcap, tight["dropped"]))
        assert tight["dropped"] > 0 and max(len(rows) for rows in tight["table"]) == tcap
        same(gpu_clip(ctx, boxes, counts, max_age, 2, tcap, match), tight, "%s, match %d, tcap %d" % (name, match, tcap))


# ------------------------------------------------------------------ 7. streams
@pytest.mark.parametrize("name", SCENES)
def test_stream_chunk_invariance(name):
    boxes, counts, tcap, max_age = setup_of(name)
    match = tar.SCENES[name][6]
    ctx = ctx_()
    ctx.stream_open(2, boxes.shape[1], track_cap=tcap)
    ref = ref_of(name, match, max_age, 2)
    for chunks in CHUNKINGS[name]:
        ctx.stream_reset([1])
        same(gpu_chunked(ctx, boxes, counts, chunks, 1, max_age, 2, tcap, match), ref, "%s, chunks %s" % (name, chunks))


@pytest.mark.parametrize("name", ["crowd_reg_grow", "crowd_lds"])
def test_slot_shared_with_the_other_entries(name):
    """assignment, best-first match, dt_associate_stream_motion, assignment on one slot: table, velocities and ids carry over every way"""
    boxes, counts, tcap, max_age = setup_of(name)
    T, cap = boxes.shape[:2]
    ctx = ctx_()
    q = max(T // 4, 1)
    chunks = [q, q, q, T - 3 * q]
    ref = tar.associate_tracks_assign_chunked(boxes, counts, THR, max_age, GAIN, 2, 0, tcap, chunks, match_at={1: BEST}, motion_at=(2,))
    assert not np.array_equal(ref["ids"], ref_of(name, 0, max_age, 2)["ids"]), "vacuous: the mixed run is the assignment's"
    ctx.stream_open(1, cap, track_cap=tcap)
    same(gpu_chunked(ctx, boxes, counts, chunks, 0, max_age, 2, tcap, 0, match_at={1: BEST}, motion_at=(2,)), ref, "assign, match, motion, assign")


def test_reset():
    ctx = ctx_()
    name = "crowd_reg_grow"
    boxes, counts, tcap, max_age = setup_of(name)
    T, cap = boxes.shape[:2]
    ref = ref_of(name, 0, max_age, 2)
    head = tar.associate_tracks_assign(boxes[:5], counts[:5], THR, max_age, GAIN, 2, 0, tcap)
    ctx.stream_open(3, cap, track_cap=tcap)
    first = gpu_chunked(ctx, boxes[:5], counts[:5], [5], 2, max_age, 2, tcap, 0)
    other = gpu_chunked(ctx, boxes[:5], counts[:5], [5], 0, max_age, 2, tcap, 0)
    same(first, head, "fresh slot")
    ctx.stream_reset([2])
    again = gpu_chunked(ctx, boxes[:5], counts[:5], [2, 3], 2, max_age, 2, tcap, 0)
    same(again, head, "the reset slot starts over")
    rest = gpu_chunked(ctx, boxes[5:], counts[5:], [T - 5], 0, max_age, 2, tcap, 0)
    same(join([other, rest]), ref, "neighbour of a reset slot")


# ------------------------------------------------------------------ 8. errors
def _code(excinfo):
    return int(re.search(r"failed \((\d+)\)", str(excinfo.value)).group(1))


def lds_bound(cap):
    """the largest tcap of the general form: 26 * tcap + 4 * cap + 6 words must not exceed 40960 (include/mi355_dt.h)"""
    return (40960 - 6 - 4 * cap) // 26


def test_errors_leave_the_state_unchanged():
    import mi355_dt
    trk, blob, tw = small_tracker()
    ctx = trk.model.ctx
    ARG, STATE = 1, 3
    name = "crowd_reg"
    boxes, counts, tcap, max_age = setup_of(name)
    T, cap = boxes.shape[:2]
    ref = ref_of(name, ANY, max_age, 2)
    b = lambda a, z: dev(boxes[None, a:z], ctx)
    c = lambda a, z: dev(counts[None, a:z], ctx)
    partial = (dict(tracks=False), dict(tinfo=False), dict(tcounts=False), dict(tracks=False, tinfo=False), dict(tinfo=False, tcounts=False),
               dict(tracks=False, tcounts=False))

    fresh = type(trk)(detector_weights=blob, tracker_weights=tw)      # no stream_open yet
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.model.ctx.associate_stream_tracks(b(0, 4), c(0, 4), THR, [0], max_age, GAIN, 2, match=ANY, assign=True)
    assert _code(e) == STATE
    fresh.model.ctx.close()

    # the stateless entry
    for bad in (dict(match=1), dict(match=3), dict(match=4), dict(match=-1), dict(min_hits=0), dict(gain=1.5), dict(gain=float("nan")),
                dict(max_age=-1), dict(track_cap=cap - 1)):
        kw = dict(max_age=max_age, gain=GAIN, min_hits=2, track_cap=tcap, match=ANY)
        kw.update(bad)
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_tracks(b(0, 4), c(0, 4), THR, kw["max_age"], kw["gain"], kw["min_hits"], track_cap=kw["track_cap"], match=kw["match"],
                                 assign=True)
        assert _code(e) == ARG, bad
    for off in partial:
        rc, o = raw_assign(ctx, b(0, 4), c(0, 4), max_age, tcap, GAIN, 2, ANY, **off)
        assert rc == ARG, off
        assert all(int((v != -7).sum()) == 0 for v in o.values() if v is not None), "a refused call wrote an output"
    # the LDS bound of the header: the bound itself runs, one entry more is refused and nothing is launched
    top = lds_bound(cap)
    assert 26 * top + 4 * cap + 6 <= 40960 < 26 * (top + 1) + 4 * cap + 6
    at = ctx.associate_tracks(b(0, 4), c(0, 4), THR, max_age, GAIN, 2, track_cap=top, match=ANY, assign=True, readout=False)
    for key in ("ids", "gaps", "hits"):
        assert np.array_equal(at[key][0].cpu().numpy(), ref[key][:4]), key
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_tracks(b(0, 4), c(0, 4), THR, max_age, GAIN, 2, track_cap=top + 1, match=ANY, assign=True, readout=False)
    assert _code(e) == ARG
    ctx.associate_tracks(b(0, 4), c(0, 4), THR, max_age, GAIN, 2, track_cap=top + 1, match=BEST | ANY, readout=False)      # (best-first fits there)
    ctx.stream_open(1, cap, track_cap=top + 1)
    with pytest.raises(mi355_dt.NativeError) as e:
        ctx.associate_stream_tracks(b(0, 4), c(0, 4), THR, [0], max_age, GAIN, 2, match=ANY, assign=True, readout=False)
    assert _code(e) == ARG
    ctx.stream_open(1, cap, track_cap=top)
    at = ctx.associate_stream_tracks(b(0, 4), c(0, 4), THR, [0], max_age, GAIN, 2, match=ANY, assign=True, readout=False)
    assert np.array_equal(at["ids"][0].cpu().numpy(), ref["ids"][:4])

    # the stream entry: refused calls between two valid ones
    ctx.stream_open(4, cap, track_cap=tcap)
    r1 = to_host(ctx.associate_stream_tracks(b(0, 5), c(0, 5), THR, [2], max_age, GAIN, 2, match=ANY, assign=True))
    for bad in (dict(match=1), dict(match=3), dict(match=4), dict(match=-1), dict(min_hits=0), dict(gain=1.5), dict(gain=float("nan")),
                dict(max_age=-1), dict(slots=[4]), dict(slots=[-1])):
        kw = dict(max_age=max_age, gain=GAIN, min_hits=2, slots=[2], match=ANY)
        kw.update(bad)
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.associate_stream_tracks(b(5, T), c(5, T), THR, kw["slots"], kw["max_age"], kw["gain"], kw["min_hits"], match=kw["match"],
                                        assign=True)
        assert _code(e) == ARG, bad
    for off in partial:
        assert raw_assign(ctx, b(5, T), c(5, T), max_age, tcap, GAIN, 2, ANY, slots=[2], **off)[0] == ARG, off
    with pytest.raises(mi355_dt.NativeError) as e:      # a slot named twice
        ctx.associate_stream_tracks(dev(boxes[None, 5:7].repeat(2, 0), ctx), dev(counts[None, 5:7].repeat(2, 0), ctx), THR, [2, 2], max_age, GAIN,
                                    2, match=ANY, assign=True)
    assert _code(e) == ARG
    with pytest.raises(mi355_dt.NativeError) as e:      # cap differs from the table's
        ctx.associate_stream_tracks(dev(boxes[None, 5:T, :cap - 1], ctx), c(5, T), THR, [2], max_age, GAIN, 2, match=ANY, assign=True)
    assert _code(e) == ARG
    n, arr = ctx._slot_array([2])
    assert ctx.lib.dt_associate_stream_tracks_assign(ctx.h, None, None, 1, 3, cap, 0.3, 3, 0.5, 2, ANY, arr, None, None, None, None, None, None,
                                                     None) == ARG
    assert ctx.lib.dt_associate_tracks_assign(ctx.h, None, None, 1, 3, cap, 0.3, 3, tcap, 0.5, 2, ANY, None, None, None, None, None, None, None) == ARG
    r2 = to_host(ctx.associate_stream_tracks(b(5, T), c(5, T), THR, [2], max_age, GAIN, 2, match=ANY, assign=True))
    same(join([r1, r2]), ref, "after the refused calls")
    alone = tar.associate_tracks_assign(boxes[5:], counts[5:], THR, max_age, GAIN, 2, ANY, tcap)
    assert not np.array_equal(ref["hits"][5:], alone["hits"]), "vacuous: the second chunk does not depend on the slot"


# ------------------------------------------------------------------ 9. the library exports the entries
def test_library_exports_the_assign_entries():
    import mi355_dt
    out = subprocess.run(["nm", "-D", "--defined-only", mi355_dt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("dt_associate_tracks_assign", "dt_associate_stream_tracks_assign"):
        assert name in exported and name in mi355_dt.SYMBOLS
    header = open(os.path.join(os.path.dirname(mi355_dt.LIB_PATH), "..", "include", "mi355_dt.h")).read()
    assert "dt_associate_tracks_assign(" in header and "dt_associate_stream_tracks_assign(" in header
    assert mi355_dt.DT_ASSIGN_IOU_SCALE == tar.ASSIGN_IOU_SCALE
    ctx = ctx_()
    assert ctx.lib.dt_abi_version() == 108
    boxes, counts = tar.worked_example()
    with pytest.raises(mi355_dt.NativeError) as e:      # 4 is no DT_MATCH_* bit: the match entries refuse it as they always did
        ctx.associate_tracks(dev(boxes[None], ctx), dev(counts[None], ctx), THR, 0, 0.0, 1, match=4)
    assert _code(e) == 1


# ------------------------------------------------------------------ 10. the tracker class
def test_tracker_with_match_optimal():
    from test_gpu_stream import small_frames, small_tracker as boxed_tracker      # (its head is scaled so that the frames carry boxes)
    trk = boxed_tracker()[0]
    ctx = trk.model.ctx
    assert not trk.MATCH_OPTIMAL
    frames = torch.from_numpy(small_frames(2, 9, seed0=360))
    trk.MATCH_OPTIMAL = True      # on the instance: the class and the other tests' tracker stay as they are
    try:
        ctx.profile_reset(); ctx.profile_enable(True)
        r = trk.track_clips(frames)
        ctx.profile_enable(False)
        assert "associate:tracks_assign" in ctx.profile_names()
        assert {"ids", "nids", "gaps", "hits"} <= set(r) and "tracks" not in r and int(r["counts"].sum()) > 0
        want = ctx.associate_tracks(r["boxes"], r["counts"], trk.ASSOC_THRESHOLD, trk.MAX_AGE, 0.0, 1, track_cap=trk.TRACK_CAP, assign=True,
                                    readout=False)
        for key in ("ids", "nids", "gaps", "hits"):
            assert torch.equal(r[key], want[key]), key
        assert set(trk.empty_result(9)) >= {"gaps", "hits"}
        trk.open_streams(3)
        ctx.profile_reset(); ctx.profile_enable(True)
        parts = [trk.track_stream(frames[:, :3], [2, 0]), trk.track_stream(frames[:, 3:], [2, 0])]
        ctx.profile_enable(False)
        assert "associate:stream_tracks_assign" in ctx.profile_names()
        boxes = torch.cat([p["boxes"] for p in parts], dim=1).contiguous()
        counts = torch.cat([p["counts"] for p in parts], dim=1).contiguous()
        want = ctx.associate_tracks(boxes, counts, trk.ASSOC_THRESHOLD, trk.MAX_AGE, 0.0, 1, track_cap=trk.TRACK_CAP, assign=True, readout=False)
        for key in ("ids", "gaps", "hits"):
            assert torch.equal(torch.cat([p[key] for p in parts], dim=1), want[key]), key
        assert torch.equal(parts[-1]["nids"], want["nids"])
        trk.MATCH_BEST_FIRST = True      # an order means nothing to an assignment: the library's refusal surfaces
        import mi355_dt
        with pytest.raises(mi355_dt.NativeError) as e:
            trk.track_clips(frames)
        assert _code(e) == 1
    finally:
        del trk.MATCH_OPTIMAL
        if "MATCH_BEST_FIRST" in vars(trk):
            del trk.MATCH_BEST_FIRST
