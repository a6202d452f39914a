"""Tiny-tracker streams on the device (dt_tiny_stream_open / _reset / _sequence / _forward).

The contract: a stream fed in chunks of any sizes gives what the stateless call gives on the concatenation of the chunks, and a
fresh slot is a stateless call -- bit for bit (torch.equal), under the default policy and the pinned one: the projection and the
head run one fixed GEMM configuration, the step's reduction tree of a track depends on neither its position nor the batch, and a
full step on h = c = 0 gives the t = 0 kernel's values.

Shapes: U = 512 (compiled in); Global pool on 4x4x32 features (D = 36, padded to 64: pad columns), one Max case at 8x8x32
(D = 132), the heatmap model at 32x32 (D = 1056, the igemm head); n in {1, 3, 70} -- 70 crosses the 64-track block of the step
and leaves a ragged group of 8; 9 frames.  The stateless results are computed once per (model, n) and shared.
"""
import functools
import re

import numpy as np
import pytest
import torch

import mi355_dt
from oracle import oracle as orc
from utility import synth

pytestmark = pytest.mark.gpu

T9 = 9
CHUNKINGS = ([9], [1] * 9, [2, 3, 4], [4, 5])
MODELS = {      # name: (fh, fw, fc, pool, heatmap size or 0)
    "global": (4, 4, 32, "Global", 0),
    "max": (8, 8, 32, "Max", 0),
    "heatmap": (4, 4, 32, "Global", 32),
}


def feat_dim(model):
    fh, fw, fc, pool, _ = MODELS[model]
    return fc if pool == "Global" else (fh // 4) * (fw // 4) * fc


def weights(model):
    hs = MODELS[model][4]
    return synth.synth_heatmap_weights(feat_dim(model), hs) if hs else synth.synth_tiny_weights(feat_dim(model))


def load(ctx, model):
    tw = weights(model)
    ctx.tiny_load(tw["kernel"].shape[0], 512, tw["kernel"], tw["recurrent"], tw["bias"], tw["dense_kernel"], tw["dense_bias"])
    return ctx


@functools.lru_cache(maxsize=None)
def model_ctx(model):
    """one context per model for the whole module; every test opens its own table (all slots fresh)"""
    return load(mi355_dt.Context(), model)


@functools.lru_cache(maxsize=None)
def inputs(model, n):
    """(feat [n,9,fh,fw,fc], det [n,9,dd]) on the host"""
    fh, fw, fc, _, hs = MODELS[model]
    rs = np.random.RandomState(1000 + n)
    feat = rs.randn(n, T9, fh, fw, fc).astype(np.float32)
    if hs:
        box = rs.rand(n * T9, 4).astype(np.float32) * [0.8, 0.8, 0.4, 0.4] + [0.1, 0.1, 0.05, 0.05]
        det = orc.heatmap_from_boxes(box.astype(np.float32), hs).reshape(n, T9, hs * hs)
    else:
        det = rs.rand(n, T9, 4).astype(np.float32)
    return feat, det


@functools.lru_cache(maxsize=None)
def stateless(model, n):
    """(x [n,9,D] rows, the stateless dt_tiny_sequence on them) -- computed once, never written"""
    ctx = model_ctx(model)
    feat, det = inputs(model, n)
    pool = MODELS[model][3]
    D = weights(model)["kernel"].shape[0]
    f = torch.from_numpy(feat).to(ctx.device)
    d = torch.from_numpy(det).to(ctx.device)
    x = ctx.tiny_features(f.reshape((n * T9,) + f.shape[2:]), d.reshape(n * T9, -1), D, pool).reshape(n, T9, D).contiguous()
    return x, ctx.tiny_sequence(x)


def run_chunks(ctx, x, chunks, slots):
    outs, t0 = [], 0
    for k in chunks:
        outs.append(ctx.tiny_stream_sequence(x[:, t0:t0 + k].contiguous(), slots))
        t0 += k
    assert t0 == x.shape[1]
    return torch.cat(outs, dim=1)


def scattered(n):
    """n distinct slots of a table of 2 n + 3, in descending order with gaps"""
    return [2 * (n - 1 - i) + 1 for i in range(n)]


# ------------------------------------------------------------------ 1. fresh slots are a stateless call
@pytest.mark.parametrize("pinned", [False, True], ids=["default", "pinned"])
@pytest.mark.parametrize("n", [1, 3, 70])
def test_fresh_slots_equal_the_stateless_call(n, pinned):
    from parallel import pinned_policy
    ctx = model_ctx("global")
    x, whole = stateless("global", n)
    with pinned_policy(ctx, on=pinned):
        ref = ctx.tiny_sequence(x) if pinned else whole
        ctx.tiny_stream_open(2 * n + 3)
        got = ctx.tiny_stream_sequence(x, scattered(n))
    assert got.shape == (n, T9, 4)
    assert torch.equal(ref, whole), "the pinned policy changed the stateless result"
    assert torch.equal(got, ref)


# ------------------------------------------------------------------ 2. chunk invariance
@pytest.mark.parametrize("chunks", CHUNKINGS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("model,n", [("global", 3), ("global", 70), ("heatmap", 3), ("heatmap", 70), ("max", 3)])
def test_chunk_invariance(model, n, chunks):
    ctx = model_ctx(model)
    x, whole = stateless(model, n)
    ctx.tiny_stream_open(2 * n + 3)
    got = run_chunks(ctx, x, chunks, scattered(n))
    assert torch.equal(got, whole)


def test_chunk_invariance_pinned():
    from parallel import pinned_policy
    ctx = model_ctx("global")
    x, whole = stateless("global", 70)
    with pinned_policy(ctx):
        ctx.tiny_stream_open(70)
        got = run_chunks(ctx, x, [2, 3, 4], list(range(70)))
    assert torch.equal(got, whole)


def test_stream_forward_is_features_then_stream_sequence():
    """dt_tiny_stream_forward (pool + concatenate inside the call), Max pool, chunks [4, 5]"""
    ctx = model_ctx("max")
    feat, det = inputs("max", 3)
    _, whole = stateless("max", 3)
    f, d = torch.from_numpy(feat).to(ctx.device), torch.from_numpy(det).to(ctx.device)
    ctx.tiny_stream_open(4)
    got = torch.cat([ctx.tiny_stream_forward(f[:, a:b].contiguous(), d[:, a:b].contiguous(), [3, 0, 1], pool="Max") for a, b in ((0, 4), (4, 9))], dim=1)
    assert torch.equal(got, whole)


# ------------------------------------------------------------------ 3. against the oracle
@pytest.mark.parametrize("model,n", [("global", 70), ("max", 3)])
def test_chunked_vs_oracle(model, n):
    ctx = model_ctx(model)
    x, _ = stateless(model, n)
    feat, det = inputs(model, n)
    ctx.tiny_stream_open(n)
    got = run_chunks(ctx, x, [2, 3, 4], list(range(n))).cpu().numpy()
    ref = orc.tinytracker_forward(feat, det, weights(model), pool=MODELS[model][3])
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-5)


# ------------------------------------------------------------------ 4. streams out of step, fresh and warm slots in one call
def test_streams_out_of_step_and_mixed_calls():
    """five streams in slots 6, 1, 4, 0, 3 of eight; seven calls, each naming another subset, every stream ends after its 9 frames.  A stream's
    outputs equal its own stateless run, so no call disturbed a slot it did not name."""
    ctx = model_ctx("global")
    n = 5
    x, whole = stateless("global", n)
    slot = [6, 1, 4, 0, 3]
    calls = [([0, 1], 2), ([1, 2, 3], 3), ([4, 0], 1), ([0, 2, 3, 4], 4), ([1], 4), ([4, 3, 2, 0], 2), ([4], 2)]
    ctx.tiny_stream_open(8)
    pos = [0] * n
    got = [[] for _ in range(n)]
    for streams, k in calls:
        xs = torch.stack([x[i, pos[i]:pos[i] + k] for i in streams]).contiguous()
        out = ctx.tiny_stream_sequence(xs, [slot[i] for i in streams])
        for r, i in enumerate(streams):
            got[i].append(out[r])
            pos[i] += k
    assert pos == [T9] * n
    for i in range(n):
        assert torch.equal(torch.cat(got[i]), whole[i]), "stream %d" % i


# ------------------------------------------------------------------ 5. reset and reload
def test_reset_one_slot_reload_and_stale_rows():
    ctx = model_ctx("global")
    x, whole = stateless("global", 3)
    ctx.tiny_stream_open(3)
    first = ctx.tiny_stream_sequence(x[:, :4].contiguous(), [0, 1, 2])
    assert torch.equal(first, whole[:, :4])
    ctx.tiny_stream_reset([1])
    xs = torch.stack([x[0, 4:], x[1, :5], x[2, 4:]]).contiguous()      # stream 1 starts again, the others go on
    second = ctx.tiny_stream_sequence(xs, [0, 1, 2])
    assert torch.equal(second[0], whole[0, 4:]) and torch.equal(second[2], whole[2, 4:])
    assert torch.equal(second[1], whole[1, :5])
    load(ctx, "global")                                                # the same weights again: every slot fresh
    assert torch.equal(ctx.tiny_stream_sequence(x[:, :2].contiguous(), [2, 0, 1]), whole[:, :2])
    ctx.tiny_stream_reset(None)
    assert torch.equal(ctx.tiny_stream_sequence(x[:, :3].contiguous(), [1, 2, 0]), whole[:, :3])
    # rows left by a stream driven with inputs of magnitude 1e30 (inf / NaN state) are not read once the slot is fresh
    wild = ctx.tiny_stream_sequence((x[:, :2] * 1e30).contiguous(), [0, 1, 2])
    ctx.tiny_stream_sequence((x[:, 2:3] * 1e30).contiguous(), [0, 1, 2])      # ... in both copies of h
    assert not bool(torch.isfinite(wild).all()) or bool((wild != whole[:, :2]).any())
    nan = ctx.tiny_stream_sequence(torch.full_like(x[:, :1], float("nan")).contiguous(), [0, 1, 2])      # NaN rows: 0 * NaN would show
    assert bool(torch.isnan(nan).all())
    ctx.tiny_stream_reset([2, 0])
    got = ctx.tiny_stream_sequence(x[[0, 2]].contiguous(), [0, 2])
    assert torch.equal(got, whole[[0, 2]])
    load(ctx, "global")
    assert torch.equal(ctx.tiny_stream_sequence(x[1:2].contiguous(), [1]), whole[1:2])


# ------------------------------------------------------------------ 6. errors
def _code(excinfo):
    return int(re.search(r"failed \((\d+)\)", str(excinfo.value)).group(1))


def test_errors_leave_the_state_unchanged():
    ARG, STATE = 1, 3
    x, whole = stateless("global", 3)
    x, whole = x[:2], whole[:2]

    bare = mi355_dt.Context()                          # no weights
    with pytest.raises(mi355_dt.NativeError) as e:
        bare.tiny_stream_open(4)
    assert _code(e) == STATE
    fresh = load(bare, "global")                       # weights, no table
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.tiny_stream_sequence(x[:, :2].contiguous(), [0, 1])
    assert _code(e) == STATE
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.tiny_stream_reset([0])
    assert _code(e) == STATE
    with pytest.raises(mi355_dt.NativeError) as e:
        fresh.tiny_stream_open(0)
    assert _code(e) == ARG
    fresh.close()

    ctx = model_ctx("global")
    ctx.tiny_stream_open(4)
    first = ctx.tiny_stream_sequence(x[:, :5].contiguous(), [2, 0])
    rest = x[:, 5:].contiguous()
    for bad in ([2, 2], [0, 4], [-1, 0]):              # duplicate, slot >= n_slots, negative
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.tiny_stream_sequence(rest, bad)
        assert _code(e) == ARG, bad
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.tiny_stream_reset(bad)
        assert _code(e) == ARG, bad
    for bad in ([2], [2, 0, 1]):                       # wrong slot count
        with pytest.raises(mi355_dt.NativeError) as e:
            ctx.tiny_stream_sequence(rest, bad)
        assert _code(e) == ARG, bad
    n, arr = ctx._slot_array([2, 0])
    out = torch.empty((2, 4, 4), dtype=torch.float32, device=ctx.device)
    assert ctx.lib.dt_tiny_stream_sequence(ctx.h, rest.data_ptr(), 2, 0, arr, out.data_ptr()) == ARG      # T = 0
    assert ctx.lib.dt_tiny_stream_sequence(ctx.h, rest.data_ptr(), 0, 4, arr, out.data_ptr()) == ARG      # n = 0
    assert ctx.lib.dt_tiny_stream_sequence(ctx.h, None, 2, 4, arr, out.data_ptr()) == ARG                 # null rows
    second = ctx.tiny_stream_sequence(rest, [2, 0])
    assert torch.equal(torch.cat([first, second], dim=1), whole), "a refused call changed a slot"


# ------------------------------------------------------------------ 7. hipGraph replay
def test_graph_replay_equals_plain_launches():
    """graphs on: three one-frame calls with a different slot list each (the plain, capture and replay paths in turn; the list is no part
    of the graph), then a fourth; against the same calls on a context without graphs"""
    x, _ = stateless("global", 3)
    ctx, plain = load(mi355_dt.Context(), "global"), model_ctx("global")
    ctx.tiny_stream_open(5); plain.tiny_stream_open(5)
    ctx.graph_enable(True)
    try:
        replays0 = ctx.profile_read("graph_replay")["launches"]
        for t, slots in enumerate(([0, 1, 2], [4, 1, 0], [1, 2, 4], [0, 4, 1])):
            xt = x[:, t:t + 1].contiguous()
            assert torch.equal(ctx.tiny_stream_sequence(xt, slots), plain.tiny_stream_sequence(xt, slots)), "call %d" % t
        assert ctx.profile_read("graph_replay")["launches"] >= replays0 + 2, "no graph was replayed"
    finally:
        ctx.graph_enable(False)
        ctx.close()


# ------------------------------------------------------------------ 8. launch account
def test_launch_account():
    ctx = model_ctx("global")
    n, T = 70, 3
    x, whole = stateless("global", n)
    ctx.tiny_stream_open(n)
    ctx.tiny_stream_sequence(x[:, :T].contiguous(), list(range(n)))      # warm
    ctx.profile_reset(); ctx.profile_enable(True)
    try:
        got = ctx.tiny_stream_sequence(x[:, T:2 * T].contiguous(), list(range(n)))
        ctx.profile_enable(False)
        assert ctx.profile_read("lstm_step")["launches"] == T
        assert ctx.profile_read("stream_state")["launches"] == (n + 63) // 64 + 1      # two slot lists of 64, one bookkeeping launch
        ctx.profile_reset(); ctx.profile_enable(True)
        ctx.tiny_sequence(x[:, :T].contiguous())
        ctx.profile_enable(False)
        assert ctx.profile_read("lstm_step")["launches"] == T            # the stateless entry launches what it did
        assert ctx.profile_read("stream_state")["launches"] == 0
    finally:
        ctx.profile_enable(False)
    assert torch.equal(got, whole[:, T:2 * T])


# ------------------------------------------------------------------ 9. end to end
def _pipeline(heatmap):
    from models_detection.KerasYOLO import KerasYOLO
    from models_tracking.TinyHeatmapTracker import TinyHeatmapTracker
    from models_tracking.TinyTracker import TinyTracker
    H = W = 64
    C, n_seq, T = 12, 3, 4
    blob = synth.synth_darknet_blob(C, head_std=0.3)
    det = KerasYOLO({'LABELS': [str(i) for i in range(C)], 'BATCH_SIZE': 4, 'IMAGE_H': H, 'IMAGE_W': W,
                     'GRID_H': 2, 'GRID_W': 2}, weights=blob)
    det.OBJ_THRESHOLD = 0.2
    cfg = {"model_tracker": {"name": "Tiny", "lstm_units": 512, "sequence_length": T, "heatmap_size": 32},
           "train": {"pool": "Global", "batch_size": 4}}
    if heatmap:
        tt = TinyHeatmapTracker(cfg, feature_dims=(4, 4, 512), weights=synth.synth_heatmap_weights(512, 32), ctx=det.model.ctx)
    else:
        tt = TinyTracker(cfg, feature_dims=(4, 4, 512), weights=synth.synth_tiny_weights(512), ctx=det.model.ctx)
    frames = np.stack([synth.synth_clip(T, H, W, 2, seed=90 + i) for i in range(n_seq)])
    return det, tt, frames


def test_tinytracker_track_stream_end_to_end():
    """TinyTracker.track_stream in chunks [1, 2, 1] against track_sequences on the 4 frames, through a StreamTable.  The detector runs at
    another batch size per chunk, so the boxes agree to the pipeline test's tolerance; under the pinned policy the detector's rows do not
    depend on the batch and the comparison is exact."""
    from models_tracking.streams import StreamTable
    from parallel import pinned_policy
    det, tt, frames = _pipeline(False)
    ctx = tt.model_tracker.ctx
    _, det4 = tt.frame_rows(frames.reshape((-1,) + frames.shape[2:]), det)
    assert int((det4.abs().sum(dim=1) > 0).sum()) > 0, "vacuous without detections"
    table = StreamTable(tt, n_slots=4, cap=10)
    keys = ["obj-%d" % i for i in range(3)]
    for k in reversed(keys):
        table.open(k)
    slots = table.slots(keys)
    assert slots == [2, 1, 0]

    def chunked():
        return torch.cat([tt.track_stream(frames[:, a:b], slots, det) for a, b in ((0, 1), (1, 3), (3, 4))], dim=1)

    whole = tt.track_sequences(frames, det)
    got = chunked()
    assert got.shape == (3, 4, 4)
    np.testing.assert_allclose(got.cpu().numpy(), whole.cpu().numpy(), rtol=1e-3, atol=1e-4)
    tt.reset_streams()
    with pinned_policy(ctx):
        whole_p = tt.track_sequences(frames, det)
        got_p = chunked()
    assert torch.equal(got_p, whole_p)


def test_tinyheatmap_track_stream_end_to_end():
    """(heat, rects) in chunks [1, 2, 1] against track_sequences: the maps to the pipeline tolerance under the default policy; under the
    pinned policy, where the detector's rows do not depend on the batch, maps and rectangles exactly"""
    from parallel import pinned_policy
    det, tt, frames = _pipeline(True)
    tt.open_streams(3)

    def chunked():
        outs = [tt.track_stream(frames[:, a:b], [1, 2, 0], det) for a, b in ((0, 1), (1, 3), (3, 4))]
        return torch.cat([o[0] for o in outs], dim=1), torch.cat([o[1] for o in outs], dim=1)

    heat, rects = tt.track_sequences(frames, det)
    got_h, got_r = chunked()
    assert got_h.shape == heat.shape == (3, 4, 1024) and got_r.shape == rects.shape == (3, 4, 4)
    assert got_r.dtype == rects.dtype == torch.int32
    np.testing.assert_allclose(got_h.cpu().numpy(), heat.cpu().numpy(), rtol=1e-3, atol=1e-4)
    tt.reset_streams()
    with pinned_policy(tt.model_tracker.ctx):
        heat_p, rects_p = tt.track_sequences(frames, det)
        got_h, got_r = chunked()
    assert torch.equal(got_h, heat_p) and torch.equal(got_r, rects_p)
    assert bool((rects_p[..., 2] >= 0).any()), "vacuous without a rectangle"
