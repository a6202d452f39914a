"""GPU suite (-m gpu): stream slots -- ConvLSTM state and track ids carried across calls.

The contract every test here states: a stream fed in chunks of any sizes gives what the stateless model gives on the
concatenation of those chunks as ONE clip -- tracking grid, boxes, counts and track ids.

  * under parallel.pinned_policy (kernel selection independent of the batch a call carries) the comparison is
    torch.equal on everything: the contract test_pinned_policy_is_batch_independent states for clips, extended along T;
  * under the default policy a call of fewer than 12 frames takes other kernel forms than a call of 30, so the
    chunked grid is held against the ORACLE on the whole sequence at the project's grid bar (tests/test_gpu_configs.py:
    per channel, max|got-ref| <= 3e-4 * max(1, max|ref|), per time step) and discrete outputs are left to the pinned tests;
  * the association carry is checked alone, bit-exact against oracle.associate_clip on the whole sequence, for both
    forms of associate_kernel (registers: every frame of the call AND the stored frame <= 64 boxes, T <= 64; LDS otherwise).
"""
import re

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from utility import synth

pytestmark = pytest.mark.gpu

KEYS = ("netout", "boxes", "counts", "ids")


def dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def chan_err(got, ref):
    """max over channels (last axis) of max|got-ref| / max(1, max|ref|) in that channel (tests/test_gpu_configs.py)"""
    g = got.reshape(-1, got.shape[-1]).astype(np.float64)
    r = ref.reshape(-1, ref.shape[-1]).astype(np.float64)
    return float((np.abs(g - r).max(0) / np.maximum(1.0, np.abs(r).max(0))).max())


def flat_c(a):
    return a.reshape(a.shape[:-2] + (-1,))


_CACHE = {}


def small_tracker():
    """96x128 (3x4 grid), C = 12, head scaled so that frames carry boxes (as __graft_entry__.smoke does)"""
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
        tw["out_kernel"] = tw["out_kernel"] * 40.0
        tw["out_bias"][4::5 + C] = 1.5
        _CACHE["small"] = (Trk(detector_weights=blob, tracker_weights=tw), blob, tw)
    return _CACHE["small"]


def small_frames(n, T, seed0=300):
    return np.stack([synth.synth_clip(T, 96, 128, 2, seed=seed0 + i) for i in range(n)])


def big_tracker():
    """416x416, calibrated by bench.build_tracker to ~32 boxes per frame, and 2 x 30 frames of bench.make_frames"""
    if "big" not in _CACHE:
        import bench
        d = torch.device("cuda", torch.cuda.current_device())
        frames = bench.make_frames(2, 30, 416, 416, d, seed0=42)
        trk, blob, tw = bench.build_tracker(416, 416, 30, 32, frames[:1])
        _CACHE["big"] = (trk, blob, tw, frames)
    return _CACHE["big"]


def run_chunks(trk, frames, chunks, slots, reset=True):
    """feed frames [n,T,..] in chunks along T; returns the concatenated result dict (nids: the last call's)"""
    assert sum(chunks) == frames.shape[1]
    if reset:
        trk.reset_streams(slots)
    parts, t0 = [], 0
    for L in chunks:
        parts.append(trk.track_stream(frames[:, t0:t0 + L], slots))
        t0 += L
    out = {k: torch.cat([p[k] for p in parts], dim=1) for k in KEYS}
    out["nids"] = parts[-1]["nids"]
    return out


def assert_same(got, ref, what, keys=KEYS + ("nids",)):
    for k in keys:
        assert got[k].shape == ref[k].shape, "%s: %s shapes %s vs %s" % (what, k, tuple(got[k].shape), tuple(ref[k].shape))
        if not torch.equal(got[k], ref[k]):
            d = (got[k].double() - ref[k].double()).abs()
            bad = d.reshape(d.shape[0], d.shape[1], -1).amax(2) > 0 if d.dim() > 1 else d > 0
            raise AssertionError("%s: %s differs (max |diff| %g) at (stream, t) = %s" % (what, k, float(d.max()), bad.nonzero().tolist()[:8]))
    assert int(ref["counts"].sum()) > 0, "%s: vacuous without boxes" % what


# ------------------------------------------------------------------ 1. fresh slots = the stateless call
@pytest.mark.parametrize("size", ["96x128", "416"])
@pytest.mark.parametrize("pinned", [False, True], ids=["default_policy", "pinned"])
def test_fresh_slots_equal_stateless_call(size, pinned):
    from parallel import pinned_policy
    if size == "416":
        trk, _, _, fr = big_tracker()
        frames, n = fr[:1], 1
    else:
        trk = small_tracker()[0]
        frames, n = small_frames(3, 4), 3
    trk.open_streams(n + 2)
    with pinned_policy(trk.model.ctx, on=pinned):
        ref = trk.track_clips(frames)
        got = trk.track_stream(frames, list(range(n)))
        again = run_chunks(trk, frames, [frames.shape[1]], list(range(n)))      # after a reset too
    assert_same(got, ref, "fresh slots")
    assert_same(again, ref, "reset slots")


# ------------------------------------------------------------------ 2. chunk invariance, bit-exact under pin
@pytest.mark.parametrize("chunks", [[30], [12, 6, 12], [1] * 30, [29, 1]], ids=["30", "12_6_12", "1x30", "29_1"])
def test_chunk_invariance_pinned_416(chunks):
    from parallel import pinned_policy
    trk, _, _, fr = big_tracker()
    trk.open_streams(2)
    with pinned_policy(trk.model.ctx):
        ref = trk.track_clips(fr[:1])
        got = run_chunks(trk, fr[:1], chunks, [1])
    assert_same(got, ref, "416, chunks %s" % chunks)


@pytest.mark.parametrize("chunks", [[12], [5, 7], [1] * 12], ids=["12", "5_7", "1x12"])
def test_chunk_invariance_pinned_small_4_streams(chunks):
    from parallel import pinned_policy
    trk = small_tracker()[0]
    frames = small_frames(4, 12)
    trk.open_streams(6)
    with pinned_policy(trk.model.ctx):
        ref = trk.track_clips(frames)
        got = run_chunks(trk, frames, chunks, [4, 0, 5, 2])
    assert_same(got, ref, "96x128, chunks %s" % chunks)


# ------------------------------------------------------------------ 3. chunked, default policy, against the oracle
def test_chunked_default_policy_vs_oracle_416():
    """(12, 6, 12) under the default policy: the 6-frame call takes the small-batch forms, the 12-frame calls the fp16 form.
    Grid bar of tests/test_gpu_configs.py, per time step; measured per-step errors are printed.  From the profile: a warm
    chunk of T frames runs T recurrent steps (t = 0 included) and no gates-only launch."""
    trk, blob, tw, fr = big_tracker()
    ctx = trk.model.ctx
    C = 12
    layers, used = orc.parse_darknet_blob(blob, C)
    assert used == blob.size
    ref = orc.tracker_forward(orc.normalize_u8(fr[0].cpu().numpy()), layers, tw)[0]      # all 30 frames as ONE clip
    trk.open_streams(1)
    parts, t0 = [], 0
    for k, L in enumerate([12, 6, 12]):
        ctx.profile_reset(); ctx.profile_enable(True)
        parts.append(trk.track_stream(fr[:1, t0:t0 + L], [0])["netout"])
        ctx.profile_enable(False)
        steps = {nm: ctx.profile_read(nm)["launches"] for nm in ctx.profile_names() if nm.endswith(":convlstm_step")}
        gates = ctx.profile_read("convlstm_gates")["launches"]
        print("chunk %d (T=%d): step launches %s, convlstm_gates %d" % (k, L, steps, gates))
        assert steps, "no launch tagged convlstm_step"
        want = L if k else L - 1
        assert all(v == want for v in steps.values()), "chunk %d of %d frames: %s, expected %d each" % (k, L, steps, want)
        assert gates == (0 if k else 1)
        t0 += L
    got = flat_c(torch.cat(parts, dim=1)[0].cpu().numpy())
    ref = flat_c(ref)
    err_t = [chan_err(got[t], ref[t]) for t in range(30)]
    print("per-step grid error vs oracle:", " ".join("%.2e" % e for e in err_t))
    assert max(err_t) <= 3e-4, "tracking grid error %g at t=%d" % (max(err_t), int(np.argmax(err_t)))


# ------------------------------------------------------------------ 4. association carry against the oracle
def moving_boxes(T, cap, n_obj_t, seed):
    """Moving boxes with births, deaths, label changes and ties (as test_associate_vs_oracle_synthetic); n_obj_t(t) = objects
    that may be alive in frame t (0: an empty frame)"""
    rs = np.random.RandomState(seed)
    n_max = max(n_obj_t(t) for t in range(T))
    pos = rs.rand(n_max, 2); vel = (rs.rand(n_max, 2) - .5) * .06; wh = rs.rand(n_max, 2) * .2 + .05
    lab = rs.randint(0, 3, n_max)
    boxes = np.zeros((T, cap, 8), dtype=np.float32)
    counts = np.zeros(T, dtype=np.int32)
    for t in range(T):
        alive = [k for k in range(n_obj_t(t)) if rs.rand() > 0.15]
        rs.shuffle(alive)
        for i, k in enumerate(alive[:cap]):
            p = pos[k] + vel[k] * t
            boxes[t, i] = [p[0], p[1], wh[k, 0], wh[k, 1], .9, lab[k] if rs.rand() > .05 else (lab[k] + 1) % 3, .8, i]
        counts[t] = min(len(alive), cap)
        if t % 5 == 3 and counts[t] >= 2:
            boxes[t, 1, :4] = boxes[t, 0, :4]      # exact duplicate -> tie on IoU
    return boxes, counts


def assoc_chunked(ctx, boxes, counts, chunks, slot, cap):
    ids, nid, t0 = [], None, 0
    for L in chunks:
        i, nid = ctx.associate_stream(dev(boxes[None, t0:t0 + L], ctx), dev(counts[None, t0:t0 + L], ctx), 0.3, [slot])
        ids.append(i[0].cpu().numpy())
        t0 += L
    assert t0 == boxes.shape[0]
    return np.concatenate(ids), int(nid[0])


ASSOC_CASES = {
    # name: (T, cap, objects alive in frame t, chunkings)
    "register_form": (40, 64, lambda t: 30, [[1] * 40, [7, 33]]),
    "lds_form_120_boxes": (8, 128, lambda t: 140, [[8], [5, 3], [1] * 8]),
    "stored_over_64_then_small": (12, 128, lambda t: 120 if t < 6 else 20, [[6, 6], [5, 1, 6]]),
    "stored_small_then_over_64": (12, 128, lambda t: 20 if t < 6 else 120, [[6, 6], [6, 1, 5]]),
    "empty_frame_at_chunk_edges": (14, 64, lambda t: 0 if t in (6, 7) else 25, [[7, 7], [6, 1, 1, 6], [8, 6]]),
    "longer_than_64_frames": (70, 32, lambda t: 12, [[40, 30], [64, 6]]),
}


@pytest.mark.parametrize("case", sorted(ASSOC_CASES))
def test_associate_stream_vs_oracle(case):
    T, cap, n_obj_t, chunkings = ASSOC_CASES[case]
    ctx = small_tracker()[0].model.ctx
    boxes, counts = moving_boxes(T, cap, n_obj_t, seed=7)
    if case == "register_form":
        assert counts.max() <= 64
    if "over_64" in case or "lds" in case:
        assert counts.max() > 64
    rid, rn = orc.associate_clip(boxes, counts, 0.3)
    assert rn > counts.max(), "vacuous: no births after frame 0"
    ctx.stream_open(3, cap)
    # a fresh slot = dt_associate
    ids0, n0 = ctx.associate_stream(dev(boxes[None], ctx), dev(counts[None], ctx), 0.3, [2])
    ids1, n1 = ctx.associate(dev(boxes[None], ctx), dev(counts[None], ctx), 0.3)
    assert torch.equal(ids0, ids1) and torch.equal(n0, n1)
    assert np.array_equal(ids0[0].cpu().numpy(), rid) and int(n0[0]) == rn
    for chunks in chunkings:
        ctx.stream_reset([1])
        ids, nid = assoc_chunked(ctx, boxes, counts, chunks, 1, cap)
        bad = np.nonzero((ids != rid).any(1))[0]
        assert bad.size == 0, "%s, chunks %s: ids differ from the oracle at frames %s" % (case, chunks, bad[:8])
        assert nid == rn, "%s, chunks %s: %d ids opened, oracle %d" % (case, chunks, nid, rn)


def test_associate_stream_5_streams_out_of_step():
    """five streams, each with its own chunking, sharing calls: a call carries the streams that have L frames left, in rotating
    order, and stream k sits out every (k + 2)-th call"""
    ctx = small_tracker()[0].model.ctx
    n, T, cap = 5, 40, 96
    seqs = [moving_boxes(T, cap, (lambda t, k=k: 10 + 18 * k), seed=20 + k) for k in range(n)]      # 10 .. 82 objects: both forms in one call
    refs = [orc.associate_clip(b, c, 0.3) for b, c in seqs]
    slot = [6, 0, 3, 8, 1]
    ctx.stream_open(9, cap)
    cur, got, nid, call = [0] * n, [[] for _ in range(n)], [0] * n, 0
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
        ids, nids = ctx.associate_stream(dev(b, ctx), dev(c, ctx), 0.3, [slot[k] for k in who])
        for j, k in enumerate(who):
            got[k].append(ids[j].cpu().numpy()); nid[k] = int(nids[j]); cur[k] += L; cuts[k].append(L)
        call += 1
    assert len({tuple(c) for c in cuts}) == n, "the streams were meant to have different chunkings: %s" % cuts
    for k in range(n):
        assert np.array_equal(np.concatenate(got[k]), refs[k][0]), "stream %d (chunks %s)" % (k, cuts[k])
        assert nid[k] == refs[k][1]


# ------------------------------------------------------------------ 5. slots are independent
def test_slots_are_independent():
    """A, B, C in slots 5, 0, 2 of 7; calls {A, B}, {C, B}, {C, A}: C is fresh while B is warm, the order in a call is permuted"""
    from parallel import pinned_policy
    trk = small_tracker()[0]
    frames = torch.from_numpy(small_frames(3, 6, seed0=340))
    A, B, C = 0, 1, 2
    slot = {A: 5, B: 0, C: 2}
    trk.open_streams(7)
    parts = {A: [], B: [], C: []}
    with pinned_policy(trk.model.ctx):
        alone = [trk.track_clips(frames[k:k + 1]) for k in (A, B, C)]
        seen = {A: 0, B: 0, C: 0}
        for who in ([A, B], [C, B], [C, A]):
            x = torch.stack([frames[k, seen[k]:seen[k] + 3] for k in who])
            r = trk.track_stream(x, [slot[k] for k in who])
            for j, k in enumerate(who):
                parts[k].append({key: r[key][j:j + 1] for key in KEYS + ("nids",)})
                seen[k] += 3
    for k in (A, B, C):
        got = {key: torch.cat([p[key] for p in parts[k]], dim=1) for key in KEYS}
        got["nids"] = parts[k][-1]["nids"]
        assert_same(got, alone[k], "stream %d" % k)


# ------------------------------------------------------------------ 6. reset and reload
def test_reset_one_slot_and_reload_weights():
    from parallel import pinned_policy
    trk, _, tw = small_tracker()
    frames = torch.from_numpy(small_frames(2, 9, seed0=360))
    trk.open_streams(4)
    with pinned_policy(trk.model.ctx):
        whole = trk.track_clips(frames)
        first = trk.track_stream(frames[:, :4], [3, 1])
        trk.reset_streams([3])
        # slot 3 starts over on its first chunk; slot 1 goes on with frames 4..7
        x = torch.stack([frames[0, :4], frames[1, 4:8]])
        second = trk.track_stream(x, [3, 1])
        for key in KEYS + ("nids",):
            assert torch.equal(second[key][0], first[key][0]), "reset slot: %s differs from its first chunk" % key
        for key in KEYS:
            assert torch.equal(torch.cat([first[key][1], second[key][1]]), whole[key][1, :8]), "neighbour of a reset slot: %s" % key
        # new tracker weights (the same values: what is checked is that no state survives the load)
        trk.model.set_weights(tw)
        third = trk.track_stream(frames[:, :4], [3, 1])
        for key in KEYS + ("nids",):
            assert torch.equal(third[key], first[key]), "after set_weights: %s differs from fresh slots" % key
    assert int(whole["counts"].sum()) > 0


# ------------------------------------------------------------------ 7. hipGraph replay
def test_graph_replay_equals_plain_launches():
    """n = 2, T = 6 at 416 (12 frames: the fp16 form), five chunks of different frames and advancing state, graphs on, against the
    same calls on a second context with graphs off"""
    trk, blob, tw, fr = big_tracker()
    plain = type(trk)(detector_weights=blob, tracker_weights=tw)
    ctx, pctx = trk.model.ctx, plain.model.ctx
    trk.open_streams(3); plain.open_streams(3)
    ctx.graph_enable(True)
    try:
        replays0 = ctx.profile_read("graph_replay")["launches"]
        for k in range(5):
            x = fr[:, 6 * k:6 * k + 6].contiguous()
            if k == 3:
                pctx.profile_reset(); pctx.profile_enable(True)
            ref = plain.track_stream(x, [2, 0])
            if k == 3:
                pctx.profile_enable(False)
                assert "s3_form:f16x2" in pctx.profile_names(), "the fp16 form did not run"
            got = trk.track_stream(x, [2, 0])
            assert_same(got, ref, "chunk %d" % k)
        assert ctx.profile_read("graph_replay")["launches"] > replays0, "no graph was replayed"
    finally:
        ctx.graph_enable(False)
        pctx.close()


# ------------------------------------------------------------------ 8. errors
def _code(excinfo):
    return int(re.search(r"failed \((\d+)\)", str(excinfo.value)).group(1))


def test_errors_leave_the_state_unchanged():
    import mi355_dt
    from parallel import pinned_policy
    trk, blob, tw = small_tracker()
    ctx = trk.model.ctx
    frames = torch.from_numpy(small_frames(2, 8, seed0=380)).to(ctx.device)
    ARG, STATE = 1, 3

    fresh = type(trk)(detector_weights=blob, tracker_weights=tw)      # no stream_open yet
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.track_stream(frames[:, :2], [0, 1])
    assert _code(e) == STATE
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.reset_streams([0])
    assert _code(e) == STATE
    fresh.model.ctx.close()

    trk.open_streams(4, cap=40)
    with pinned_policy(ctx):
        whole = trk.track_clips(frames, cap=40)
        first = trk.track_stream(frames[:, :5], [2, 0])
        for bad in ([2, 2], [0, 4], [-1, 0]):
            with pytest.raises(mi355_dt.NativeError) as e:
                trk.track_stream(frames[:, 5:], bad)
            assert _code(e) == ARG, bad
            with pytest.raises(mi355_dt.NativeError) as e:
                ctx.associate_stream(first["boxes"], first["counts"], 0.3, bad)
            assert _code(e) == ARG, bad
        with pytest.raises(mi355_dt.NativeError) as e:      # cap differs from the table's
            ctx.associate_stream(first["boxes"][:, :, :39].contiguous(), first["counts"], 0.3, [2, 0])
        assert _code(e) == ARG
        n, arr = ctx._slot_array([2, 0])
        assert ctx.lib.dt_track_stream_forward(ctx.h, None, 0, 2, 3, arr, None, None) == ARG      # null frames
        assert ctx.lib.dt_associate_stream(ctx.h, None, None, 2, 3, 40, 0.3, arr, None, None) == ARG
        second = trk.track_stream(frames[:, 5:], [2, 0])
    got = {k: torch.cat([first[k], second[k]], dim=1) for k in KEYS}
    got["nids"] = second["nids"]
    assert_same(got, whole, "after the refused calls")
