"""GPU suite: the max-|x| slots of the fp16 form (dt_internal.h: dt_ctx::amax, dt_amax_publish; network.hip: amax_note / ensure_amax).

The fp16 form scales every operand by a power of two from the max |x| of its tensor.  Inside a forward nothing measures that
maximum: the kernel that wrote the tensor publishes it from its epilogue and the host links the slot to the tensor by pointer-range
tags.  The scale depends on the maximum's exponent only, so a wrong word costs precision (too high) or overflows fp16 on the rare
elements near the maximum (too low) -- invisible to the network tests' tolerances.  These tests read the slots (dt_amax_read) and
  (a) under DT_AMAX_MEASURE=1, where every fp16-form consumer measures its input into its own slot, require the measured word to
      be bit-equal to the word the producer published, for every producing epilogue;
  (b) compare published / measured words with max |x| of the tensor on the host;
  (c) require bit-identical results with the producers' words and with measured ones, with and without graph replay;
  (d) require that no slot state leaks from one call into the next."""
import numpy as np
import pytest
import torch

from utility import synth
from test_gpu_parity import _detector, _tracker, dev

pytestmark = pytest.mark.gpu

SLOT_IN, SLOT_TRK, SLOT_TEST = 32, 56, 57

# the slot a consumer conv_j reads its input's max |x| from when the producer published it: the previous layer's output (conv_4's
# for conv_5 also when conv_4 runs inside conv_3's launch, conv_13's POOLED output for conv_14), the concat for conv_22 (slot 20:
# conv_20's 1024 channels + the space_to_depth channels added by the cat_skip pass), conv_feat for conv_23.  conv_21 reads the
# unpooled skip tensor, which nothing tags: it is not listed.
PRODUCER = {j: j - 1 for j in range(2, 21)}
PRODUCER.update({22: 20, 23: 22})


def _bits(v):
    return int(np.asarray(v, dtype=np.float32).view(np.uint32))


def _host_amax(t):
    """max |x| of a device tensor, NaNs skipped (as fmaxf does in the kernels), as float32"""
    a = t.detach().float().abs()
    a = torch.where(torch.isnan(a), torch.zeros_like(a), a)
    return np.float32(a.max().item()) if a.numel() else np.float32(0.0)


def _slots(c, idx):
    return {i: c.amax_read(i) for i in idx}


def _absmax_tags(c):
    """the consumers that measured their input in the profiled calls: {'conv_22': n, 'trk': n, 'cat_skip': n, ...}"""
    return {n.split(":", 1)[1]: c.profile_read(n)["launches"] for n in c.profile_names()
            if n.startswith("absmax:") and c.profile_read(n)["launches"]}


def _profiled(c, fn):
    c.profile_reset(); c.profile_enable(True)
    out = fn()
    c.profile_enable(False)
    return out, set(c.profile_names())


def _producer_family(names, p):
    """the kernel family whose epilogue wrote (and published) conv_p's output, from the profile"""
    if p == 1:
        return "conv1_direct:bf16" if "conv1_direct:bf16" in names else None
    if p == 4 and "conv_direct_h2:fused_1x1" in names and not any(n.endswith(":conv_4") for n in names):
        return "conv_direct_h2+1x1"
    if "wino_output:conv_%d" % p in names:      # (the Winograd GEMM itself is tagged conv_gemm_s3 / conv_igemm too)
        return "wino_output"
    fam = [f for f in ("conv_direct_h2", "conv_fused", "conv_gemm_s3", "conv_igemm") if "%s:conv_%d" % (f, p) in names]
    assert len(fam) == 1, (p, fam)
    return fam[0]


# ------------------------------------------------------------------ (a) published word == measured word, per producer kind
# (mode id, environment, H, W, frames): between them every publishing epilogue runs (test_modes_cover_every_epilogue)
MODES = [
    ("default_12", {}, 416, 416, 12),
    ("default_16", {}, 416, 416, 16),
    ("default_48", {}, 416, 416, 48),
    ("c3h2_nofuse", {"DT_C3H2": "2", "DT_C3FUSE": "0"}, 416, 416, 12),
    ("c3h2_fuse", {"DT_C3H2": "2", "DT_C3FUSE": "1"}, 416, 416, 12),
    ("fused4", {"DT_C3H2": "0", "DT_WINO_FUSED4": "2"}, 416, 416, 12),
    ("igemm", {"DT_WINO": "0", "DT_S3_1X1_MINROWS": "0"}, 416, 416, 12),
    ("wino_f4", {"DT_WINO": "2", "DT_WINO_TILE": "4"}, 416, 416, 12),
    ("wino_f6", {"DT_WINO": "2", "DT_WINO_TILE": "6"}, 416, 416, 12),
    ("s3_1x1", {"DT_S3": "2", "DT_S3_1X1_MINROWS": "0", "DT_S3_1X1_MINK": "0"}, 416, 416, 12),
    ("odd_default", {}, 96, 160, 12),
    ("odd_forced", {"DT_WINO": "2", "DT_C3H2": "2", "DT_S3": "2", "DT_S3_1X1_MINROWS": "0"}, 96, 160, 12),
]
MODE = {m[0]: m[1:] for m in MODES}

# recorded on the MI355X: per mode, the consumers conv_j whose measured input word was compared with a published one, those whose
# producer published nothing (they measure in the default policy too), and the kernel families that published the compared words.
# A change of kernel selection shows up here first: re-record it deliberately.
EXPECTED = {
    'default_12': dict(pairs=[2, 6, 7, 8, 9, 14, 19, 20, 22], unpublished=[11, 13, 16, 18],
                            kinds=['conv1_direct:bf16', 'conv_gemm_s3', 's2d:conv_igemm', 'wino_output']),
    'default_16': dict(pairs=[2, 6, 7, 8, 9, 14, 19, 20, 22], unpublished=[11, 13, 16, 18],
                            kinds=['conv1_direct:bf16', 'conv_gemm_s3', 's2d:conv_igemm', 'wino_output']),
    'default_48': dict(pairs=[2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 19, 20, 22], unpublished=[16, 18],
                            kinds=['conv1_direct:bf16', 'conv_direct_h2', 'conv_direct_h2+1x1', 'conv_gemm_s3', 's2d:conv_igemm', 'wino_output']),
    'c3h2_nofuse': dict(pairs=[2, 3, 5, 6, 7, 8, 9, 14, 19, 20, 22], unpublished=[11, 13, 16, 18],
                             kinds=['conv1_direct:bf16', 'conv_direct_h2', 'conv_gemm_s3', 'conv_igemm', 's2d:conv_igemm', 'wino_output']),
    'c3h2_fuse': dict(pairs=[2, 3, 5, 6, 7, 8, 9, 14, 19, 20, 22], unpublished=[11, 13, 16, 18],
                           kinds=['conv1_direct:bf16', 'conv_direct_h2', 'conv_direct_h2+1x1', 'conv_gemm_s3', 's2d:conv_igemm', 'wino_output']),
    'fused4': dict(pairs=[7, 9, 14, 19, 20, 22], unpublished=[11, 13, 16, 18],
                        kinds=['conv_fused', 's2d:conv_igemm', 'wino_output']),
    'igemm': dict(pairs=[2, 7], unpublished=[10, 12],
                       kinds=['conv1_direct:bf16', 'conv_igemm']),
    'wino_f4': dict(pairs=[2, 7], unpublished=[],
                         kinds=['conv1_direct:bf16', 'wino_output']),
    'wino_f6': dict(pairs=[2, 6, 7, 8, 9, 14, 19, 20, 22], unpublished=[11, 13, 16, 18],
                         kinds=['conv1_direct:bf16', 'conv_gemm_s3', 's2d:conv_igemm', 'wino_output']),
    's3_1x1': dict(pairs=[2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 23], unpublished=[],
                        kinds=['conv1_direct:bf16', 'conv_direct_h2', 'conv_gemm_s3', 's2d:conv_igemm', 'wino_output']),
    'odd_default': dict(pairs=[6, 8], unpublished=[],
                             kinds=['conv_igemm', 'wino_output']),
    'odd_forced': dict(pairs=[2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 23], unpublished=[],
                            kinds=['conv1_direct:bf16', 'conv_direct_h2', 'conv_direct_h2+1x1', 'conv_gemm_s3', 's2d:conv_igemm', 'wino_output']),
}


def _compare_mode(monkeypatch, env, H, W, B, seed=5):
    """one forward in the default policy and one under DT_AMAX_MEASURE=1 on a fresh context; returns what was compared"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("DT_AMAX_MEASURE", raising=False)
    det, _, _ = _detector(None, H, W, 12)
    c = det.model.ctx
    frames = dev(synth.synth_clip(B, H, W, 3, seed=seed), c)
    (net0, feat0), names0 = _profiled(c, lambda: c.detect_forward(frames, want_feat=True))
    meas0 = _absmax_tags(c)
    pub0 = _slots(c, range(1, 24))
    monkeypatch.setenv("DT_AMAX_MEASURE", "1")
    c.reload_policy()
    (net1, feat1), names1 = _profiled(c, lambda: c.detect_forward(frames, want_feat=True))
    meas1 = _absmax_tags(c)
    s = _slots(c, range(0, 64))
    monkeypatch.delenv("DT_AMAX_MEASURE")
    c.reload_policy()
    # the producers publish the same words whether or not the consumers look at them, and the consumers scale by the same powers of two
    assert {i: _bits(v) for i, v in pub0.items()} == {i: _bits(s[i]) for i in range(1, 24)}
    assert torch.equal(net0, net1) and torch.equal(feat0, feat1)
    assert _bits(s[0]) == _bits(1.0)
    consumers = sorted(int(k[5:]) for k in meas1 if k.startswith("conv_"))
    assert set(meas1) - {"cat_skip"} == {"conv_%d" % j for j in consumers}, meas1
    pairs, unpublished, kinds = [], [], set()
    for j in consumers:
        assert j in PRODUCER, "conv_%d measured an input no producer tags" % j
        p = PRODUCER[j]
        if _bits(s[p]) == 0:
            unpublished.append(j)       # (split-K, a form without a publishing epilogue): the consumer must measure in the default policy too
            continue
        assert _bits(s[SLOT_IN + j]) == _bits(s[p]), "conv_%d: measured %r, producer published %r into slot %d" % (j, s[SLOT_IN + j], s[p], p)
        pairs.append(j)
        kinds.add(_producer_family(names1, p))
        if j == 22:      # the concat: conv_20's channels and the space_to_depth channels of conv_21 (its own slot, 4 x 64 columns)
            assert _bits(s[SLOT_IN + 22]) == _bits(max(s[20], s[21])), (s[SLOT_IN + 22], s[20], s[21])
            if _bits(s[21]):
                kinds.add("s2d:" + _producer_family(names1, 21))
    # the default policy measures exactly where no producer published: a tag that fails to match shows up as an extra measurement
    assert set(meas0) - {"cat_skip"} == {"conv_%d" % j for j in unpublished}, (meas0, unpublished)
    # (the cat_skip pass completes slot 20 wherever conv_20 published, whether or not conv_22 then reads it in the fp16 form)
    assert ("cat_skip" in meas0) == ("cat_skip" in meas1) == (_bits(s[20]) != 0), (meas0, meas1, s[20])
    assert 22 not in consumers or (22 in pairs) == (_bits(s[20]) != 0)
    return dict(pairs=pairs, unpublished=unpublished, kinds=sorted(k for k in kinds if k))


@pytest.mark.parametrize("mode", [m[0] for m in MODES])
def test_published_word_equals_measured_word(monkeypatch, mode):
    got = _compare_mode(monkeypatch, *MODE[mode])
    assert len(got["pairs"]) >= 2, got
    assert got == EXPECTED[mode], (mode, got)


def test_modes_cover_every_epilogue():
    """the coverage claim of MODES, checked against the recorded table: every kernel family that publishes ran as a producer"""
    assert set(EXPECTED) == set(MODE)
    kinds = set().union(*(set(e["kinds"]) for e in EXPECTED.values()))
    for k in ("conv1_direct:bf16", "conv_direct_h2", "conv_direct_h2+1x1", "conv_fused", "wino_output", "conv_igemm", "conv_gemm_s3",
              "s2d:conv_igemm"):
        assert k in kinds, (k, sorted(kinds))


# ------------------------------------------------------------------ (b) published / measured words vs max |x| on the host
# (layer name for dt_detector_extract, the slot its producer publishes into): pooled outputs, plain outputs, space_to_depth, concat
EXTRACT_TAPS = [("max_pooling2d_2", 2), ("max_pooling2d_3", 5), ("max_pooling2d_4", 8), ("max_pooling2d_5", 13), ("leaky_re_lu_4", 4),
                ("leaky_re_lu_9", 9), ("leaky_re_lu_10", 10), ("leaky_re_lu_14", 14), ("leaky_re_lu_19", 19), ("lambda_1", 21),
                ("concatenate_1", 20)]
EXTRACT_EXPECTED = {      # recorded on the MI355X: per mode, the taps whose slot was published (and compared)
    'default_12': ['max_pooling2d_2', 'max_pooling2d_3', 'max_pooling2d_4', 'max_pooling2d_5', 'leaky_re_lu_4', 'leaky_re_lu_9', 'leaky_re_lu_14', 'leaky_re_lu_19', 'lambda_1', 'concatenate_1', 'conv_feat:22', 'conv_feat:22'],
    'igemm': ['max_pooling2d_2', 'max_pooling2d_3', 'max_pooling2d_4', 'max_pooling2d_5', 'leaky_re_lu_4', 'leaky_re_lu_10', 'lambda_1'],
    'wino_f4': ['max_pooling2d_2', 'max_pooling2d_3', 'max_pooling2d_4', 'max_pooling2d_5', 'leaky_re_lu_4', 'leaky_re_lu_9', 'leaky_re_lu_14', 'leaky_re_lu_19', 'lambda_1', 'concatenate_1', 'conv_feat:22', 'conv_feat:22'],
    'fused4': ['max_pooling2d_2', 'max_pooling2d_3', 'max_pooling2d_4', 'max_pooling2d_5', 'leaky_re_lu_4', 'leaky_re_lu_9', 'leaky_re_lu_14', 'leaky_re_lu_19', 'lambda_1', 'concatenate_1', 'conv_feat:22', 'conv_feat:22'],
    'odd_forced': ['max_pooling2d_2', 'max_pooling2d_3', 'max_pooling2d_4', 'max_pooling2d_5', 'leaky_re_lu_4', 'leaky_re_lu_9', 'leaky_re_lu_10', 'leaky_re_lu_14', 'leaky_re_lu_19', 'lambda_1', 'concatenate_1', 'conv_feat:22', 'conv_feat:22', 'conv_feat:55'],
}


def _compare_extract(monkeypatch, mode):
    """the taps' slots against max |x| of the tapped tensors; returns the taps whose slot was published"""
    env, H, W, B = MODE[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    det, _, _ = _detector(None, H, W, 12)
    c = det.model.ctx
    frames = dev(synth.synth_clip(B, H, W, 3, seed=6), c)
    compared = []
    for name, slot in EXTRACT_TAPS:
        out = c.detector_extract(frames, name)
        v = c.amax_read(slot)
        if _bits(v):
            assert _bits(v) == _bits(_host_amax(out)), (name, v, _host_amax(out))
            compared.append(name)
    # conv_feat: published by conv_22's epilogue into slot 22 (or measured by conv_23 into 32 + 23 under DT_AMAX_MEASURE)
    for measure in ("0", "1"):
        monkeypatch.setenv("DT_AMAX_MEASURE", measure)
        c.reload_policy()
        c.detect_forward_internal(frames)
        feat = _host_amax(c.detector_tap("conv_feat", B))
        for slot in (22, SLOT_IN + 23):
            v = c.amax_read(slot)
            if _bits(v) and (slot == 22 or measure == "1"):
                assert _bits(v) == _bits(feat), (slot, v, feat)
                compared.append("conv_feat:%d" % slot)
    monkeypatch.delenv("DT_AMAX_MEASURE")
    c.reload_policy()
    return compared


@pytest.mark.parametrize("mode", ["default_12", "igemm", "wino_f4", "fused4", "odd_forced"])
def test_published_words_match_host(monkeypatch, mode):
    compared = _compare_extract(monkeypatch, mode)
    assert len(compared) >= 4, compared
    assert compared == EXTRACT_EXPECTED[mode], (mode, compared)


def test_tracker_slot_matches_z_rows(monkeypatch):
    """the ConvLSTM input projection's slot 56 against max |x| of the z rows dt_track_detect hands out for the same frames: measured in the
    two-step form (z carries conv_23's x_bbox columns: no producer slot describes the whole row), and in the merged form (the 1024 conv_feat
    columns) equal to conv_22's published word under DT_AMAX_MEASURE"""
    H, W, T, n = 416, 416, 4, 3
    trk, _, _ = _tracker(H, W, T)
    c = trk.model.ctx
    d = dev(np.stack([synth.synth_clip(T, H, W, 2, seed=30 + i) for i in range(n)]), c)
    z = c.track_detect(d.reshape(n * T, H, W, 3).contiguous())
    monkeypatch.setenv("DT_TRK_MERGE", "0")
    c.reload_policy()
    _profiled(c, lambda: c.track_forward(d, want_det=False))
    assert _absmax_tags(c).get("trk") == 1
    assert _bits(c.amax_read(SLOT_TRK)) == _bits(_host_amax(z)), (c.amax_read(SLOT_TRK), _host_amax(z))
    monkeypatch.setenv("DT_TRK_MERGE", "1")
    monkeypatch.setenv("DT_AMAX_MEASURE", "1")
    c.reload_policy()
    _, names = _profiled(c, lambda: c.track_forward(d, want_det=False))
    assert "convlstm_xproj:merged_conv23" in names and _absmax_tags(c).get("trk") == 1
    feat = _host_amax(z[..., :1024])
    assert _bits(c.amax_read(SLOT_TRK)) == _bits(feat) == _bits(c.amax_read(22)), (c.amax_read(SLOT_TRK), feat, c.amax_read(22))
    monkeypatch.delenv("DT_AMAX_MEASURE")
    c.reload_policy()
    _profiled(c, lambda: c.track_forward(d, want_det=False))
    assert "trk" not in _absmax_tags(c)         # the default policy takes conv_22's word for the merged projection


ADVERSARIAL = ["last_element", "negative_max", "zeros", "subnormals", "negative_zero", "one_nan", "ragged"]


@pytest.mark.parametrize("case", ADVERSARIAL)
def test_test_entry_slot_matches_host(ctx, monkeypatch, case):
    """dt_conv2d in the fp16 form measures its caller's tensor into slot 57: the word must be the host's max |x| for inputs where a
    reduction goes wrong (the maximum in the last element, a negative maximum, zeros of either sign, subnormals only, one NaN -- skipped
    -- and a pixel count that is no multiple of any block)"""
    monkeypatch.setenv("DT_S3_H2", "1")
    monkeypatch.setenv("DT_WINO", "2")
    monkeypatch.setenv("DT_WINO_TILE", "6")
    monkeypatch.setenv("DT_S3", "2")
    rs = np.random.RandomState(ADVERSARIAL.index(case))
    B, H, W, Cin, Cout = (20, 7, 11, 96, 128) if case == "ragged" else (20, 13, 13, 128, 128)
    x = (rs.randn(B, H, W, Cin) * 0.5).astype(np.float32)
    if case == "last_element":
        x.flat[-1] = 6.5
    elif case == "negative_max":
        x.flat[x.size // 3] = -11.0
    elif case == "zeros":
        x[:] = 0.0
    elif case == "subnormals":
        x = (x * np.float32(1e-39)).astype(np.float32)
        assert np.abs(x).max() < np.finfo(np.float32).tiny and np.abs(x).max() > 0
    elif case == "negative_zero":
        x = np.full_like(x, -0.0)
    elif case == "one_nan":
        x.flat[777] = np.nan
    elif case == "ragged":
        x.flat[-5] = -3.75
    w = (rs.randn(3, 3, Cin, Cout) / np.sqrt(9 * Cin)).astype(np.float32)
    xd = dev(x, ctx)
    _, names = _profiled(ctx, lambda: ctx.conv2d(xd, w, None, leaky_slope=1.0, pool=0))
    assert ctx.profile_read("absmax:test")["launches"] == 1 and ctx.profile_read("s3_form:f16x2")["launches"] == 1, sorted(names)
    want = _host_amax(xd)
    assert _bits(ctx.amax_read(SLOT_TEST)) == _bits(want), (ctx.amax_read(SLOT_TEST), want)


# ------------------------------------------------------------------ (c) the consumers read the right slot: measured scales give the same bits
C_EXTRACT = ("max_pooling2d_4", "leaky_re_lu_19", "concatenate_1", "conv_feat")


@pytest.mark.parametrize("graphs", [False, True], ids=["plain", "graphs"])
@pytest.mark.parametrize("H,W,B", [(416, 416, 12), (416, 416, 16), (416, 416, 24), (608, 608, 12), (96, 160, 12)])
def test_measured_scales_give_the_same_bits(monkeypatch, H, W, B, graphs):
    n_clips, T = 4, B // 4
    trk, _, _ = _tracker(H, W, T)
    c = trk.model.ctx
    d = dev(np.stack([synth.synth_clip(T, H, W, 2, seed=80 + i) for i in range(n_clips)]), c)
    flat = d.reshape(B, H, W, 3).contiguous()
    one = dev(synth.synth_clip(30, H, W, 2, seed=90)[None], c)
    reps = 3 if graphs else 1      # with graphs: plain launches, capture, replay -- after every policy change (it drops the graphs)

    def run():
        r = {}
        c.graph_enable(graphs)
        try:
            replays = c.profile_read("graph_replay")["launches"]
            for i in range(reps):
                c.detect_forward_internal(flat)
                r["netout", i] = c.detector_tap("conv_23", B)
                r["conv_feat", i] = c.detector_tap("conv_feat", B)
            for merge in ("1", "0"):
                monkeypatch.setenv("DT_TRK_MERGE", merge)
                c.reload_policy()
                for i in range(reps):
                    r["track_merge" + merge, i] = c.track_forward(d, want_det=False)
            monkeypatch.delenv("DT_TRK_MERGE")
            c.reload_policy()
            for i in range(reps):
                r["one_clip", i] = c.track_forward(one, want_det=False)
            for layer in C_EXTRACT:
                r[layer, 0] = c.detector_extract(flat, layer)
            if graphs:
                assert c.profile_read("graph_replay")["launches"] > replays
        finally:
            c.graph_enable(False)
        for (k, i), v in r.items():
            assert torch.equal(v, r[k, 0]), (k, i)      # captured and replayed = plain launches
        return r

    base = run()
    monkeypatch.setenv("DT_AMAX_MEASURE", "1")
    c.reload_policy()
    meas = run()
    monkeypatch.delenv("DT_AMAX_MEASURE")
    c.reload_policy()
    for k in base:
        assert torch.equal(base[k], meas[k]), k


# ------------------------------------------------------------------ (d) no slot state leaks from one call into the next
def test_no_slot_state_leaks_between_calls():
    """A forward on frames B gives the bits -- and leaves the slot words -- of the same forward on a fresh context, whatever ran before
    it: a forward on frames A with larger activations (a slot not zeroed per forward keeps A's maxima), a forward below DT_H2_MINFRAMES,
    the layer-level entry points, taps and the recurrent half, and a trunk graph captured on A and replayed on B."""
    H = W = 416
    n_clips, T = 4, 3
    Bn = n_clips * T
    rs = np.random.RandomState(17)
    frames_a = rs.randint(0, 256, (Bn, H, W, 3)).astype(np.uint8)                                  # full-range noise
    frames_b = (synth.synth_clip(Bn, H, W, 2, seed=18) // 4 + 96).astype(np.uint8)              # dim, low contrast
    ref, _, _ = _tracker(H, W, T)
    rc = ref.model.ctx
    want_net, want_feat = rc.detect_forward(dev(frames_b, rc), want_feat=True)
    want = _slots(rc, range(64))
    trk, _, _ = _tracker(H, W, T)
    c = trk.model.ctx
    da, db = dev(frames_a, c), dev(frames_b, c)

    def check(what):
        net, feat = c.detect_forward(db, want_feat=True)
        got = _slots(c, range(64))
        assert torch.equal(net, want_net) and torch.equal(feat, want_feat), what
        diff = [i for i in range(64) if (i < SLOT_IN or _bits(want[i])) and _bits(got[i]) != _bits(want[i])]
        assert not diff, (what, [(i, got[i], want[i]) for i in diff])

    c.detect_forward(da)
    a_slots = _slots(c, range(24))
    assert any(_bits(a_slots[i]) > _bits(want[i]) for i in range(1, 24)), "frames A must raise some slot above B's"
    check("after a forward on other frames")
    c.detect_forward(da[:11].contiguous())
    check("after a forward of 11 frames")
    x = dev(rs.randn(2, 13, 13, 128).astype(np.float32), c)
    c.conv2d(x, (rs.randn(3, 3, 128, 128) * 0.03).astype(np.float32), None, leaky_slope=0.1, pool=0)
    U = 32
    c.convlstm_step(dev(rs.randn(2, 13, 13, 64).astype(np.float32), c), dev(rs.randn(2, 13, 13, U).astype(np.float32) * 0.5, c),
                    dev(rs.randn(2, 13, 13, U).astype(np.float32), c), (rs.randn(3, 3, 64, 4 * U) * 0.05).astype(np.float32),
                    (rs.randn(3, 3, U, 4 * U) * 0.05).astype(np.float32), rs.randn(4 * U).astype(np.float32))
    c.detector_extract(da, "leaky_re_lu_13")
    c.detect_forward_internal(da)
    c.detector_tap("conv_feat", Bn)
    z = c.track_detect(da)
    c.track_recurrent(z.reshape((n_clips, T) + tuple(z.shape[1:])).contiguous())
    check("after the layer-level entry points, taps and the recurrent half")
    c.graph_enable(True)
    try:
        c.detect_forward(da)                # plain launches
        c.detect_forward(da)                # captured
        replays = c.profile_read("graph_replay")["launches"]
        check("replayed on B after a capture on A")
        assert c.profile_read("graph_replay")["launches"] > replays
    finally:
        c.graph_enable(False)
