"""GPU suite, part 8 (-m gpu): the result of a call does not depend on what the context ran before it.

A context keeps its device workspaces from call to call (network.hip: ws_get never clears a buffer that is large enough) and several kernels
read columns or rows of them that nobody writes: the pad channels of the tracker's z rows and of the LSTM's staged x rows, the rows Mt..Mp of
the split GEMM's operand, the split-K slabs.  Every case here runs one target call twice -- on a fresh context, and on a context that has
first run the SAME entry point at a larger shape on float32 input full of +inf, -inf, NaN and 3e38 (and, for the network entry points,
has been reconfigured for another class count / D / image size / Winograd tile and back) -- and asserts

  1. the fresh result is finite and within the oracle bar tests/test_gpu_parity.py holds that kernel form to,
  2. the result on the used context is the fresh one bit for bit,
  3. the polluting calls ran the kernel form the case is about (profile tag) and their own output is not finite.

The library accepts dt_detector_config / dt_tracker_load / dt_tiny_load on a live context (it does not refuse a second configuration), so the
reconfiguration cases assert the results, not a refusal.  Nothing non-finite goes to decode, association or target encoding; no graphs; the
stream slots (explicit carried state) are not part of this.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from utility import synth
import mi355_dt

pytestmark = pytest.mark.gpu

ANCHORS = [0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828]
NET_TOL = 3e-4                      # tests/test_gpu_parity.py: whole-network bar on chan_err
NONFINITE = (np.inf, -np.inf, np.nan, 3e38)


def relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def chan_err(got, ref):
    g = got.reshape(-1, got.shape[-1]).astype(np.float64)
    r = ref.reshape(-1, ref.shape[-1]).astype(np.float64)
    return float((np.abs(g - r).max(0) / np.maximum(1.0, np.abs(r).max(0))).max())


def flat_c(a):
    return a.reshape(a.shape[:-2] + (-1,))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def poison(a, frame_axes=1):
    """float32 [frames..., H, W, C] with +inf, -inf, NaN and 3e38 in four pixels of every frame and all over one whole frame"""
    a = np.array(a, dtype=np.float32)
    n = int(np.prod(a.shape[:frame_axes]))
    f = a.reshape(n, -1, a.shape[-1])
    for k, v in enumerate(NONFINITE):
        f[:, (5 + 11 * k) % f.shape[1], :] = v
        f[n // 2, k::4, :] = v
    return a


def assert_history_free(make_ctx, pollute, target, oracle_check):
    """target(c) -> {name: numpy array} on a fresh context (finite, within the oracle's bar) and on a context pollute(c) has used before:
    the same bits.  pollute(c) returns the outputs of its own calls: some of them must not be finite, or it polluted nothing."""
    fresh = make_ctx()
    try:
        want = target(fresh)
    finally:
        fresh.close()
    for k in sorted(want):
        assert np.isfinite(want[k]).all(), "%s: the fresh context's result is not finite" % k
    oracle_check(want)
    live = make_ctx()
    try:
        left = pollute(live)
        got = target(live)
    finally:
        live.close()
    assert left and any(not np.isfinite(a).all() for a in left), "the polluting calls left nothing non-finite behind: vacuous"
    for k in sorted(want):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if g.tobytes() == w.tobytes():
            continue
        bad = np.flatnonzero(g.view(np.uint32).ravel() != w.view(np.uint32).ravel())
        first = np.unravel_index(int(bad[0]), g.shape)
        with np.errstate(invalid="ignore"):
            d = np.abs(g.astype(np.float64) - w.astype(np.float64)).ravel()[bad]
        raise AssertionError("%s depends on the context's history: %d of %d values differ, first at %s (got %r, fresh %r), max |diff| %s, %d of them not finite"
                             % (k, bad.size, g.size, tuple(int(i) for i in first), g[first], w[first],
                                np.nanmax(d) if np.isfinite(d).any() else "n/a", int((~np.isfinite(g.ravel()[bad])).sum())))


def polluter(tags, *steps):
    """the steps (c -> list of numpy outputs, one per polluting call) under the profile; every one of those outputs must hold a non-finite value -- a step
    that left none polluted nothing; tags: {profile name: least number of launches, 0 = must not have run}"""
    def run(c):
        c.profile_reset(); c.profile_enable(True)
        outs = []
        for i, s in enumerate(steps):
            o = s(c)
            assert o and all(not np.isfinite(a).all() for a in o), "polluting step %d: an output of its calls is all finite -- vacuous" % i
            outs += o
        c.profile_enable(False)
        for name, least in sorted(tags.items()):
            n = c.profile_read(name)["launches"]
            assert (n >= least) if least else n == 0, "polluter: %s ran %d times (wanted %s); recorded: %s" % (
                name, n, ">= %d" % least if least else "0", c.profile_names())
        return outs
    return run


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------------------------- dt_conv2d
def _conv_data(shape, seed):
    B, H, W, Cin, k, Cout, pool = shape
    rs = np.random.RandomState(seed)
    x = rs.randn(B, H, W, Cin).astype(np.float32)
    w = (rs.randn(k, k, Cin, Cout) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    b = rs.randn(Cout).astype(np.float32)
    return x, w, b


WINO2 = {"DT_WINO": "2"}
S3 = {"DT_WINO": "2", "DT_WINO_TILE": "6", "DT_S3": "2"}
# id: (policy, target (B, H, W, Cin, k, Cout, pool), polluter shape, parity bar on relerr, polluter's profile tags)
# The polluters: more frames and another K, so that the workspaces exist and are larger -- 48 frames of 13x13 are 294 F(6x6) tiles (3x3 mosaics), above the
# target's 27 tiles rounded up to the split GEMM's 256 rows; the direct and the fused kernel exist for conv_2 / 3 / 5's channel counts only: more and larger frames
CONV_CASES = {
    "wino_F2": (dict(WINO2, DT_WINO_TILE="2", DT_S3="0"), (3, 13, 13, 96, 3, 384, 0), (48, 13, 13, 128, 3, 384, 0), 2e-5, {"wino_input": 1, "wino_output": 1, "conv_gemm_s3": 0}),
    "wino_F4": (dict(WINO2, DT_WINO_TILE="4", DT_S3="0"), (3, 13, 13, 96, 3, 384, 0), (48, 13, 13, 128, 3, 384, 0), 1e-4, {"wino_input": 1, "wino_output": 1, "conv_gemm_s3": 0}),
    "wino_F6": (dict(WINO2, DT_WINO_TILE="6", DT_S3="0"), (3, 13, 13, 96, 3, 384, 0), (48, 13, 13, 128, 3, 384, 0), 2e-4, {"wino_input": 1, "wino_output": 1, "conv_gemm_s3": 0}),
    "s3_f16x2": (dict(S3, DT_S3_H2="1", DT_S3_HALF="0"), (3, 13, 13, 96, 3, 384, 0), (48, 13, 13, 128, 3, 384, 0), 2e-4, {"conv_gemm_s3": 1, "s3_form:f16x2": 1, "s3_tile:256": 1}),
    "s3_bf16x3": (dict(S3, DT_S3_H2="0", DT_S3_HALF="0"), (3, 13, 13, 96, 3, 384, 0), (48, 13, 13, 128, 3, 384, 0), 2e-4, {"conv_gemm_s3": 1, "s3_form:bf16x3": 1, "s3_tile:256": 1}),
    "s3_f16x2_half": (dict(S3, DT_S3_H2="1", DT_S3_HALF="1"), (3, 13, 13, 128, 3, 256, 0), (48, 13, 13, 192, 3, 256, 0), 2e-4, {"conv_gemm_s3": 1, "s3_form:f16x2": 1, "s3_tile:128x2": 1}),
    "s3_bf16x3_half": (dict(S3, DT_S3_H2="0", DT_S3_HALF="1"), (3, 13, 13, 128, 3, 256, 0), (48, 13, 13, 192, 3, 256, 0), 2e-4, {"conv_gemm_s3": 1, "s3_form:bf16x3": 1, "s3_tile:128x2": 1}),
    "1x1_f16x2": ({"DT_S3": "2", "DT_S3_H2": "1"}, (16, 13, 13, 256, 1, 128, 0), (40, 13, 13, 512, 1, 128, 0), 1e-4, {"conv_gemm_s3": 1, "s3_form:f16x2": 1}),
    "1x1_bf16x3": ({"DT_S3": "2", "DT_S3_H2": "0"}, (16, 13, 13, 256, 1, 128, 0), (40, 13, 13, 512, 1, 128, 0), 1e-4, {"conv_gemm_s3": 1, "s3_form:bf16x3": 1}),
    "direct_h2": ({"DT_C3H2": "2", "DT_WINO_FUSED4": "2"}, (2, 26, 22, 64, 3, 128, 0), (5, 40, 44, 64, 3, 128, 0), 5e-6, {"conv_direct_h2": 1, "absmax": 1}),
    "direct_h2_pool": ({"DT_C3H2": "2", "DT_WINO_FUSED4": "2"}, (3, 32, 48, 32, 3, 64, 1), (7, 48, 64, 32, 3, 64, 1), 5e-6, {"conv_direct_h2": 1, "absmax": 1}),
    "fused_F4": ({"DT_WINO_FUSED4": "2", "DT_C3H2": "0"}, (2, 26, 22, 64, 3, 128, 0), (5, 40, 44, 64, 3, 128, 0), 1e-4, {"conv_fused": 1, "wino_input": 0}),
    "fused_F4_pool": ({"DT_WINO_FUSED4": "2", "DT_C3H2": "0"}, (3, 32, 48, 32, 3, 64, 1), (7, 48, 64, 32, 3, 64, 1), 1e-4, {"conv_fused": 1, "wino_input": 0}),
    "split_k": ({}, (1, 13, 13, 512, 3, 1024, 0), (3, 13, 13, 768, 3, 1024, 0), 2e-5, {"splitk_reduce": 1}),
    "igemm_n_edge": ({}, (3, 13, 13, 96, 1, 85, 0), (8, 13, 13, 128, 1, 85, 0), 2e-5, {"conv_igemm": 1, "conv_gemm_s3": 0}),
}


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv2d_is_history_free(monkeypatch, case):
    env, shape, big, tol, tags = CONV_CASES[case]
    set_env(monkeypatch, env)
    pool = shape[6]
    x, w, b = _conv_data(shape, 11)
    ref = orc.conv2d(x, w, b)
    ref = np.where(ref > 0, ref, ref * np.float32(0.1)).astype(np.float32)
    if pool:
        ref = orc.maxpool2(ref)
    px, pw, pb = _conv_data(big, 12)
    px = poison(px)

    def target(c):
        return {"out": c.conv2d(dev(x), w, b, leaky_slope=0.1, pool=pool).cpu().numpy()}

    def check(want):
        e = relerr(want["out"], ref)
        print("%s: relerr %.3g (bar %g)" % (case, e, tol))
        assert e < tol, e

    assert_history_free(mi355_dt.Context, polluter(tags, lambda c: [c.conv2d(dev(px), pw, pb, leaky_slope=0.1, pool=big[6]).cpu().numpy()]), target, check)


# ---------------------------------------------------------------------------------------------------------------- dt_convlstm_step
def _lstm_data(B, H, W, Cx, U, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(B, H, W, Cx).astype(np.float32)
    h = (rs.randn(B, H, W, U) * .5).astype(np.float32)
    c = rs.randn(B, H, W, U).astype(np.float32)
    Wk = (rs.randn(3, 3, Cx, 4 * U) * .05).astype(np.float32)
    Uk = (rs.randn(3, 3, U, 4 * U) * .05).astype(np.float32)
    b = (rs.randn(4 * U) * .1).astype(np.float32)
    return x, h, c, Wk, Uk, b


# id: (policy, atol of the parity test of that form at this shape (rtol 1e-4), polluter's tags)
CONVLSTM_CASES = {
    "xproj_F6_s3": ({"DT_WINO": "2", "DT_S3": "2", "DT_S3_HALF": "0"}, 1e-4, {"conv_gemm_s3:convlstm_xproj": 1, "wino_output": 2}),
    "step_F4_s3": ({"DT_WINO": "2", "DT_S3": "2", "DT_S3_HALF": "1", "DT_WINO_TILE": "4"}, 1e-4, {"conv_gemm_s3:convlstm_step": 1, "wino_output": 2}),
    "F6_fp32": ({"DT_WINO": "2", "DT_S3": "0"}, 1e-4, {"wino_output": 2, "conv_gemm_s3": 0}),
    "F4_fp32": ({"DT_WINO": "2", "DT_S3": "0", "DT_WINO_TILE": "4"}, 5e-5, {"wino_output": 2, "conv_gemm_s3": 0}),
}


@pytest.mark.parametrize("case", sorted(CONVLSTM_CASES))
def test_convlstm_step_is_history_free(monkeypatch, case):
    env, atol, tags = CONVLSTM_CASES[case]
    set_env(monkeypatch, env)
    x, h, cc, Wk, Uk, b = _lstm_data(6, 13, 13, 64, 32, 19)
    rh, rc = orc.convlstm_step(x, h, cc, Wk, Uk, b)
    px, ph, pc, pWk, pUk, pb = _lstm_data(40, 13, 13, 96, 64, 20)      # more frames (3x3 mosaics: 245 tiles), other K and N
    px = poison(px)

    def run(c, *a):
        return [t.cpu().numpy() for t in c.convlstm_step(dev(a[0]), dev(a[1]), dev(a[2]), a[3], a[4], a[5])]

    def check(want):
        np.testing.assert_allclose(want["h"], rh, rtol=1e-4, atol=atol)
        np.testing.assert_allclose(want["c"], rc, rtol=1e-4, atol=atol)

    assert_history_free(mi355_dt.Context, polluter(tags, lambda c: run(c, px, ph, pc, pWk, pUk, pb)),
                        lambda c: dict(zip(("h", "c"), run(c, x, h, cc, Wk, Uk, b))), check)


# ---------------------------------------------------------------------------------------------------------------- detector, tracker
H, W, C = 64, 96, 12


@functools.lru_cache(maxsize=None)
def _blob(nb_class):
    return synth.synth_darknet_blob(nb_class, seed=1234)


@functools.lru_cache(maxsize=None)
def _layers(nb_class):
    layers, used = orc.parse_darknet_blob(_blob(nb_class), nb_class)
    assert used == _blob(nb_class).size
    return layers


@functools.lru_cache(maxsize=None)
def _tracker_weights(nb_class, units):
    return synth.synth_tracker_weights(nb_class, units=units, seed=1235 + nb_class)


def _configure(c, h, w, nb_class, units=None):
    """(re)configure a context -- fresh or live -- for a detector of nb_class classes and, with units, its tracker head"""
    c.detector_config(h, w, 5, nb_class, ANCHORS)
    assert c.load_darknet_weights(_blob(nb_class)) == _blob(nb_class).size
    if units:
        tw = _tracker_weights(nb_class, units)
        c.tracker_load(units, tw["kernel"], tw["recurrent"], tw["bias"], tw["out_kernel"], tw["out_bias"])
    return c


def _noise_frames(n, h, w, seed):
    """float32 frames in [0, 1], poisoned"""
    return poison(np.random.RandomState(seed).rand(n, h, w, 3).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _detect_reference():
    frames = synth.synth_clip(5, H, W, 3, seed=31)
    net, feat, _ = orc.yolov2_forward(orc.normalize_u8(frames), _layers(C))
    return frames, net, feat


DET_POLICIES = {
    "default": ({}, {"conv1_direct": 1, "conv_igemm": 1}),
    "winograd": ({"DT_WINO": "2", "DT_WINO_FUSED4": "2"}, {"wino_input": 1, "conv_fused": 1}),
    "direct_h2": ({"DT_WINO": "2", "DT_WINO_FUSED4": "2", "DT_C3H2": "2", "DT_H2_MINFRAMES": "0"}, {"wino_input": 1, "conv_direct_h2:fused_1x1": 1}),
}


def _detect_big(c, h=H, w=W):
    return [c.detect_forward(dev(_noise_frames(12, h, w, 41))).cpu().numpy()]


def _detect_other_size(c):
    """image 96x64 on the live context, then 64x96 again: every activation workspace keeps its size and changes its geometry"""
    _configure(c, W, H, C)
    out = _detect_big(c, W, H)
    _configure(c, H, W, C)
    return out


def _detect_other_tiles(monkeypatch):
    """DT_WINO_TILE 6, 4, 2 on the live context (the tile is applied when weights are loaded), then the policy of the case again"""
    def step(c):
        out = []
        for ts in ("6", "4", "2"):
            monkeypatch.setenv("DT_WINO_TILE", ts)
            c.reload_policy()
            _configure(c, H, W, C)
            out += _detect_big(c)
        monkeypatch.delenv("DT_WINO_TILE")
        c.reload_policy()
        _configure(c, H, W, C)
        return out
    return step


# every policy and frame type after the larger forward; the reconfigurations where they can matter: another image size under the default policy,
# other Winograd tiles where Winograd runs
DET_CASES = [(p, d, "big") for p in sorted(DET_POLICIES) for d in ("uint8", "float32")] + \
            [(p, d, h) for p, h in (("default", "other_size"), ("winograd", "other_tiles")) for d in ("uint8", "float32")]


@pytest.mark.parametrize("policy,dtype,history", DET_CASES, ids=["-".join(c) for c in DET_CASES])
def test_detect_forward_is_history_free(monkeypatch, policy, dtype, history):
    """5 frames of 64x96 (below DT_H2_MINFRAMES: the polluter's 12 frames take the fp16 forms and publish max-|x| slots the target must not see)."""
    env, tags = DET_POLICIES[policy]
    set_env(monkeypatch, env)
    frames, ref_net, ref_feat = _detect_reference()
    x = frames if dtype == "uint8" else orc.normalize_u8(frames)

    def target(c):
        net, feat = c.detect_forward(dev(x), want_feat=True)
        return {"netout": net.cpu().numpy(), "feat": feat.cpu().numpy()}

    def check(want):
        e = chan_err(flat_c(want["netout"]), flat_c(ref_net)), chan_err(want["feat"], ref_feat)
        print("%s %s: chan_err %.3g / %.3g (bar %g)" % (policy, dtype, e[0], e[1], NET_TOL))
        assert max(e) < NET_TOL, e

    steps = {"big": [_detect_big], "other_size": [_detect_big, _detect_other_size], "other_tiles": [_detect_big, _detect_other_tiles(monkeypatch)]}[history]
    assert_history_free(lambda: _configure(mi355_dt.Context(), H, W, C), polluter(tags, *steps), target, check)


N_CLIPS, T, U = 3, 4, 512


@functools.lru_cache(maxsize=None)
def _track_reference():
    clips = np.stack([synth.synth_clip(T, H, W, 2, seed=20 + i) for i in range(N_CLIPS)])
    refs = [orc.tracker_forward(orc.normalize_u8(clips[i]), _layers(C), _tracker_weights(C, U)) for i in range(N_CLIPS)]
    return clips, np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])


TRK_POLICIES = {
    "default": ({}, None, {"convlstm_gates": 1}),
    "split": ({"DT_WINO": "2", "DT_S3": "2"}, None, {"convlstm_gates": 1, "s3_form:f16x2": 1, "conv_gemm_s3:convlstm_step": 1}),
    "pin": ({}, 1, {"convlstm_gates": 1, "s3_form:bf16x3": 1, "s3_form:f16x2": 0, "convlstm_xproj:merged_conv23": 0}),
}


def _track_make(pin):
    def make():
        c = mi355_dt.Context()
        if pin is not None:
            c.policy_set("pin", pin)
        return _configure(c, H, W, C, U)
    return make


def _track_big(c, n_clips=5, t=5):
    frames = _noise_frames(n_clips * t, H, W, 43).reshape(n_clips, t, H, W, 3)
    return [o.cpu().numpy() for o in c.track_forward(dev(frames), want_det=True)]


def _track_other_classes(c):
    """dt_tracker_load for 80 classes (z rows of 1472 floats: 1449 + 23 pad) and 64 units on the live context, a forward, and the 12-class model
    (rows of 1120: 1109 + 11 pad, on bytes that held the other model's activations) again"""
    _configure(c, H, W, 80, 64)
    out = _track_big(c, 4, 4)
    _configure(c, H, W, C, U)
    return out


def _track_other_size(c):
    """image 96x64 (grid 3x2) on the live context, then 64x96 (grid 2x3) again"""
    _configure(c, W, H, C, U)
    frames = _noise_frames(16, W, H, 44).reshape(4, 4, W, H, 3)
    out = [o.cpu().numpy() for o in c.track_forward(dev(frames), want_det=True)]
    _configure(c, H, W, C, U)
    return out


def _track_other_tiles(monkeypatch):
    """DT_WINO_TILE 6, 4, 2 on the live context (64 units: the reload is cheap), then the policy and the model of the case again"""
    def step(c):
        out = []
        for ts in ("6", "4", "2"):
            monkeypatch.setenv("DT_WINO_TILE", ts)
            c.reload_policy()
            _configure(c, H, W, C, 64)
            out += _track_big(c, 4, 4)
        monkeypatch.delenv("DT_WINO_TILE")
        c.reload_policy()
        _configure(c, H, W, C, U)
        return out
    return step


# (under the pin the merged input projection is off whatever DT_TRK_MERGE says: one case)
TRK_CASES = [(p, m, "big") for p, m in (("default", "1"), ("default", "0"), ("split", "1"), ("split", "0"), ("pin", "0"))] + \
            [(p, m, "other_classes") for p, m in (("default", "1"), ("default", "0"), ("split", "1"), ("split", "0"), ("pin", "0"))] + \
            [("default", "0", "other_size"), ("split", "1", "other_tiles")]


@pytest.mark.parametrize("policy,merge,history", TRK_CASES, ids=["%s-merge%s-%s" % c for c in TRK_CASES])
def test_track_forward_is_history_free(monkeypatch, policy, merge, history):
    """3 clips x 4 frames of 64x96, 12 classes, 512 units (12 frames: the fp16 forms run, slot 56 measures the z rows)."""
    env, pin, tags = TRK_POLICIES[policy]
    set_env(monkeypatch, dict(env, DT_TRK_MERGE=merge))
    if policy == "split":
        tags = dict(tags, **{"convlstm_xproj:merged_conv23": 1 if merge == "1" else 0})
    clips, ref_trk, ref_det = _track_reference()

    def target(c):
        trk, det = c.track_forward(dev(clips), want_det=True)
        return {"trk": trk.cpu().numpy(), "det": det.cpu().numpy()}

    def check(want):
        e = [max(chan_err(flat_c(want[k][i]), flat_c(r[i])) for i in range(N_CLIPS)) for k, r in (("trk", ref_trk), ("det", ref_det))]
        print("%s merge %s: chan_err trk %.3g det %.3g (bar %g)" % (policy, merge, e[0], e[1], NET_TOL))
        assert max(e) < NET_TOL, e

    steps = [_track_big] + {"big": [], "other_classes": [_track_other_classes], "other_size": [_track_other_size],
                            "other_tiles": [_track_other_tiles(monkeypatch)]}[history]
    assert_history_free(_track_make(pin), polluter(tags, *steps), target, check)


# ---------------------------------------------------------------------------------------------------------------- TinyTracker
@functools.lru_cache(maxsize=None)
def _tiny_weights(feat_dim):
    return synth.synth_tiny_weights(feat_dim, seed=1236 + feat_dim)


def _tiny_load(c, feat_dim):
    tw = _tiny_weights(feat_dim)
    c.tiny_load(feat_dim + 4, 512, tw["kernel"], tw["recurrent"], tw["bias"], tw["dense_kernel"], tw["dense_bias"])
    return c


# feature map (fh, fw, fc), pool mode -> pooled width: D = width + 4, staged in rows of D rounded up to 32
TINY_SHAPES = {"global_516": ((13, 13, 512), "Global", 512), "max_132": ((8, 8, 32), "Max", 128), "global_512": ((13, 13, 508), "Global", 508)}


def _tiny_big(shape):
    (fh, fw, fc), pool, _ = TINY_SHAPES[shape]

    def step(c):
        rs = np.random.RandomState(51)
        feat = poison(rs.randn(9, 4, fh, fw, fc).astype(np.float32), frame_axes=2)
        return [c.tiny_forward(dev(feat), dev(rs.rand(9, 4, 4).astype(np.float32)), pool=pool).cpu().numpy()]
    return step


def _tiny_other_d(other, back):
    """dt_tiny_load for another D on the live context, a forward in that model's pool mode, and the case's own weights again"""
    def step(c):
        _tiny_load(c, TINY_SHAPES[other][2])
        out = _tiny_big(other)(c)
        _tiny_load(c, TINY_SHAPES[back][2])
        return out
    return step


# id: (target entry, its shape, the other model of the reconfiguration or None)
TINY_CASES = {
    "forward_global_516": ("forward", "global_516", None),
    "forward_global_516_after_D_512": ("forward", "global_516", "global_512"),      # rows of 512 floats, no pad -> rows of 544: 516 + 28 pad
    "forward_max_132": ("forward", "max_132", None),
    "forward_max_132_after_D_516": ("forward", "max_132", "global_516"),            # rows of 544 -> rows of 160: 132 + 28 pad
    "sequence_516": ("sequence", "global_516", None),
    "sequence_512_after_D_516": ("sequence", "global_512", "global_516"),           # rows of 544 -> rows of 512
    "sequence_132_after_D_516": ("sequence", "max_132", "global_516"),
}


@pytest.mark.parametrize("case", sorted(TINY_CASES))
def test_tiny_tracker_is_history_free(case):
    entry, shape, other = TINY_CASES[case]
    (fh, fw, fc), pool, width = TINY_SHAPES[shape]
    rs = np.random.RandomState(11)
    feat = rs.randn(5, 3, fh, fw, fc).astype(np.float32)
    det = rs.rand(5, 3, 4).astype(np.float32)
    ref = orc.tinytracker_forward(feat, det, _tiny_weights(width), pool=pool)
    # dt_tiny_sequence takes the pooled rows: a maximum is exact, so the oracle's pooling gives the rows dt_tiny_features would
    pooled = (orc.global_maxpool if pool == "Global" else orc.maxpool4_flatten)(feat.reshape(15, fh, fw, fc)).reshape(5, 3, width)
    rows = np.concatenate([pooled, det], axis=2)

    def target(c):
        if entry == "forward":
            return {"out": c.tiny_forward(dev(feat), dev(det), pool=pool).cpu().numpy()}
        return {"out": c.tiny_sequence(dev(rows)).cpu().numpy()}

    steps = [_tiny_big(shape)] + ([_tiny_other_d(other, shape)] if other else [])
    assert_history_free(lambda: _tiny_load(mi355_dt.Context(), width), polluter({"pool": 1, "lstm_step": 1, "conv_igemm:lstm_xproj": 1}, *steps), target,
                        lambda want: np.testing.assert_allclose(want["out"], ref, rtol=1e-4, atol=2e-5))
