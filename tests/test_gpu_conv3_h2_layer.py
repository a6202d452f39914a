"""GPU suite: the direct fp16-form 3x3 kernel (csrc/conv3_h2.hip) at LAYER level -- its persistent item loop and its fused 1x1 tail.

The kernel is launched as min(items, 2 x CUs) workgroups that walk the items (frame, tile, channel tile) with stride gridDim.x.  From
its second item on a workgroup runs code its first item never runs: the next item's patch is requested during stage 0, taps 7 and 8
refill the weight ring with the NEXT item's stages 0 and 1, the accumulators are cleared again, and in the FUSE instance (conv_3 with
conv_4's 1x1 applied to the tile before it leaves the CU) the ring base rotates by 13 % 3 = 1 per item.  The other layer-level tests stay
below 2 x CUs items, so all of that used to be judged 20 layers later at the whole-network bar only.

  A. test_item_loop_turns_over: ctx.conv2d at shapes whose batch is sized FROM the device's CU count so that every (distinct frame,
     tile) pair is computed at turn 0 and at a later turn, and some workgroup runs four items.  Every distinct frame against the oracle
     at the kernel's own bar (5e-6), and every repeat of a frame bit-equal to its first copy: a frame's result does not depend on the
     workgroup or the turn that computed it (the operand scale comes from the whole tensor's max |x|, the same for every item).
  B. test_fused_*: dt_detector_extract("leaky_re_lu_4") IS the fused launch's output wherever the forward fuses.  Reference: conv_3 +
     BN + LeakyReLU + conv_4 + BN + LeakyReLU in float64 of the DEVICE's own max_pooling2d_2 (so conv_1 / conv_2 arithmetic never
     enters).  The bar is not chosen here: it is 4 x the largest error U of the TWO-launch form (DT_C3FUSE=0: the same kernel without
     FUSE + the separate 1x1 GEMM) against the same reference over these cases, recorded in profiles/c3h2_layer_tests.txt.

The item map the premises restate (conv3_h2.hip: unit_of, c3_launch): item = (frame * tiles + tile) * ntn + channel tile, with
tiles = ceil(H / TH) * ceil(W / 16), TH = 8 for 128 output channels and 16 for 64, ntn = 1 for every shape the kernel accepts
(Cout <= 128); workgroup = item % G, turn = item // G, G = 2 x CUs as soon as items >= G.  A test whose premise does not hold on the
device it runs on FAILS (it does not skip): a part with another CU count needs another batch formula, and the test must say so.

Not reachable, hence untested: the bias reload at `nxt.n0 != cur.n0` (one channel tile per item: Cout <= 128), the `N1 < 64` guards of
the fused tail (conv_4 has 64 outputs), and a partial tile ROW in the FUSE instance (conv_3 runs at H / 4 of a frame height that is a
multiple of 32: always whole 8-row tiles; partial rows are covered on the plain instances in A)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from utility import synth
from test_gpu_parity import chan_err, dev, relerr

pytestmark = pytest.mark.gpu

C = 12                      # classes of the synthetic detector (conv_23 only)
LEAKY = np.float32(0.1)
BN_EPS = np.float32(1e-3)

# 4 x the largest error U of the two-launch form against the float64 reference, measured on the MI355X (profiles/c3h2_layer_tests.txt
# holds U and the fused form's error per case), per class of case so that the engineered one does not loosen the others:
#   FUSED_BAR      the cases on the synthetic detector's own weights (conv_4 a 128-term sum): largest U 2.50e-6
#   SELECTION_BAR  conv_4 as a signed selection behind a conv_3 whose channels 0..63 are 64 times smaller than the others: in BOTH forms
#                  conv_3's error follows the tensor's largest value, so those channels carry 64 times the relative error
#                  (largest U 5.96e-6, the odd channels)
# Both lie below the 5e-5 the whole-network comparison already gives.  Not to be widened to make a case pass.
FUSED_BAR = 1.0e-5
SELECTION_BAR = 2.3e-5


def _workgroups(ctx):
    return 2 * torch.cuda.get_device_properties(ctx.device).multi_processor_count


def _assert_turnover(B, K, tiles, G, min_items):
    """the coverage premise, from the kernel's item map: frames b = d, d + K, d + 2K, ... carry distinct frame d; every (d, tile) pair is
    computed at turn 0 and at some turn >= 1, and some workgroup runs at least `min_items` items.  Returns the turns each d is seen at."""
    items = B * tiles                                   # ntn == 1
    assert items > G, "the launch has %d workgroups for %d items: the loop never turns over" % (G, items)
    it = np.arange(items)
    frame, tile, wg, turn = it // tiles, it % tiles, it % G, it // G
    key = (frame % K) * tiles + tile
    first, later = np.zeros(K * tiles, bool), np.zeros(K * tiles, bool)
    first[key[turn == 0]] = True
    later[key[turn >= 1]] = True
    assert first.all(), "distinct (frame, tile) pairs never computed as a workgroup's first item: %s" % np.flatnonzero(~first)[:8]
    assert later.all(), "distinct (frame, tile) pairs never computed at a later turn: %s" % np.flatnonzero(~later)[:8]
    assert np.bincount(wg).max() >= min_items, "no workgroup runs %d items (%d items, %d workgroups)" % (min_items, items, G)
    return [set(turn[(frame % K) == d].tolist()) for d in range(K)]


# ---------------------------------------------------------------------------------------------------------------- A. the item loop
@pytest.mark.parametrize("H,W,Cin,Cout,pool", [
    (8, 16, 64, 128, 0),      # WN = 2 plain: one whole tile per frame, two chunks -- chunk turn-over and item turn-over interleave
    (10, 12, 64, 128, 1),     # WN = 2 pooled: two tile rows, the second of 2 rows; a partial column
    (16, 16, 32, 64, 1),      # WN = 1 pooled: conv_2's class, one chunk
    (13, 13, 64, 64, 0),      # WN = 1 plain: odd, smaller than a tile
    (20, 36, 32, 128, 0),     # WN = 2 plain: 3 x 3 tiles per frame -- a workgroup's consecutive items are different tiles of different frames
])
def test_item_loop_turns_over(ctx, monkeypatch, H, W, Cin, Cout, pool):
    monkeypatch.setenv("DT_C3H2", "2")
    G = _workgroups(ctx)
    TH = 8 if Cout % 128 == 0 else 16
    tiles = -(-H // TH) * -(-W // 16)
    assert -(-Cout // (128 if Cout % 128 == 0 else 64)) == 1      # ntn
    K = min(64, G // tiles)                                   # distinct frames: all of their tiles fit into turn 0
    B = max(-(-(3 * G + 1) // tiles), -(-G // tiles) + K)     # items >= 3 G + 1, and a whole set of K frames lies past turn 0
    assert K >= 8 and B * tiles >= 3 * G + 1
    _assert_turnover(B, K, tiles, G, 3)

    rs = np.random.RandomState(H * 1000 + W * 10 + Cin + Cout + pool)
    distinct = rs.randn(K, H, W, Cin).astype(np.float32)
    w = (rs.randn(3, 3, Cin, Cout) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = rs.randn(Cout).astype(np.float32)
    ref = orc.conv2d(distinct, w, b)
    ref = np.where(ref > 0, ref, ref * LEAKY).astype(np.float32)
    if pool:
        ref = orc.maxpool2(ref)
    idx = torch.arange(B, device=ctx.device) % K
    x = dev(distinct, ctx)[idx].contiguous()
    ctx.profile_reset(); ctx.profile_enable(True)
    got = ctx.conv2d(x, w, b, leaky_slope=0.1, pool=pool)
    ctx.profile_enable(False)
    assert ctx.profile_read("conv_direct_h2")["launches"] == 1 and ctx.profile_read("conv_fused")["launches"] == 0
    # the first copies (turn 0) and the last K frames (the highest turns) against the oracle, frame by frame; every frame in between is
    # covered by the bit-equality with its first copy below
    head = got[:K].cpu().numpy()
    tail = got[B - K:].cpu().numpy()
    e_head = max(relerr(head[d], ref[d]) for d in range(K))
    e_tail = max(relerr(tail[j], ref[(B - K + j) % K]) for j in range(K))
    print("c3h2_layer item_loop %dx%d %d->%d pool=%d: G=%d K=%d B=%d items=%d err first=%.3g last=%.3g"
          % (H, W, Cin, Cout, pool, G, K, B, B * tiles, e_head, e_tail))
    assert e_head < 5e-6 and e_tail < 5e-6, (e_head, e_tail)
    same = (got == got[:K][idx]).flatten(1).all(1)
    assert bool(same.all()), "frames whose bits differ from their first copy: %s" % torch.nonzero(~same).flatten()[:16].tolist()


# ---------------------------------------------------------------------------------------------------------------- B. the fused 1x1
def _detector_from(blob, H, W):
    from models_detection.KerasYOLO import KerasYOLO
    det = KerasYOLO({'LABELS': [str(i) for i in range(C)], 'BATCH_SIZE': 4, 'IMAGE_H': H, 'IMAGE_W': W, 'GRID_H': H // 32,
                     'GRID_W': W // 32}, weights=blob)
    layers, used = orc.parse_darknet_blob(blob, C)
    assert used == blob.size
    return det.model.ctx, layers


def _sections(blob):
    """views into a darknet blob: {layer: dict(beta, gamma, mean, var, kernel [O, I, k, k])}, walking synth.FILE_ORDER"""
    out, off = {}, 4
    for (i, k, ci, co) in synth.FILE_ORDER:
        s = {}
        for name in ("beta", "gamma", "mean", "var"):
            s[name] = blob[off:off + co]; off += co
        s["kernel"] = blob[off:off + co * ci * k * k].reshape(co, ci, k, k); off += co * ci * k * k
        out[i] = s
    return out


def _frames(n, H, W, seed):
    """uint8 frames: moving-rectangle clips (smooth) on the even indices, noise on the odd ones"""
    f = synth.synth_clip(n, H, W, 3, seed=seed)
    f[1::2] = np.random.RandomState(seed).randint(0, 256, size=f[1::2].shape).astype(np.uint8)
    return f


def _fold(L):
    scale = L["gamma"].astype(np.float64) / np.sqrt(L["var"].astype(np.float64) + np.float64(BN_EPS))
    return scale, L["beta"].astype(np.float64) - L["mean"].astype(np.float64) * scale


def _ref_conv34(p2, layers, last=4):
    """float64: LeakyReLU(BN(conv_4(LeakyReLU(BN(conv_3(p2)))))) of a float32 NHWC tensor (last=3: conv_3's block alone)"""
    F = torch.nn.functional
    x = torch.from_numpy(np.ascontiguousarray(p2)).double().permute(0, 3, 1, 2)
    for i, pad in ((3, 1), (4, 0))[:last - 2]:
        L = layers[i]
        s, t = _fold(L)
        wk = torch.from_numpy(np.ascontiguousarray(L["kernel"])).double().permute(3, 2, 0, 1)      # HWIO -> OIHW
        x = F.conv2d(x, wk, padding=pad) * torch.from_numpy(s)[None, :, None, None] + torch.from_numpy(t)[None, :, None, None]
        x = torch.where(x > 0, x, x * float(LEAKY))
    return x.permute(0, 2, 3, 1).contiguous().numpy()


def _extract(c, frames, fused):
    """leaky_re_lu_4 by extraction, with the launches it must consist of"""
    c.profile_reset(); c.profile_enable(True)
    out = c.detector_extract(frames, "leaky_re_lu_4")
    c.profile_enable(False)
    conv4 = [n for n in c.profile_names() if n.endswith(":conv_4") and not n.startswith("absmax:") and c.profile_read(n)["launches"]]
    if fused:
        assert c.profile_read("conv_direct_h2:fused_1x1")["launches"] == 1 and not conv4, conv4
    else:      # the direct kernel without FUSE, conv_4 in a launch of its own
        assert c.profile_read("conv_direct_h2:fused_1x1")["launches"] == 0 and c.profile_read("conv_direct_h2:conv_3")["launches"] == 1
        assert len(conv4) == 1 and c.profile_read(conv4[0])["launches"] == 1, conv4
    return out


def _fused_and_unfused(c, monkeypatch, frames):
    p2 = c.detector_extract(frames, "max_pooling2d_2")
    fused = _extract(c, frames, True)
    monkeypatch.setenv("DT_C3FUSE", "0")
    c.reload_policy()
    unfused = _extract(c, frames, False)
    monkeypatch.delenv("DT_C3FUSE")
    c.reload_policy()
    return p2, fused, unfused


def _judge(case, fused, unfused, ref, bar=FUSED_BAR):
    """fused / unfused / ref: numpy [n, h, w, 64].  Prints U (two-launch form vs float64), the fused form's error and fused vs unfused"""
    assert fused.shape == ref.shape == unfused.shape and ref.shape[-1] == 64
    u, f, fu = chan_err(unfused, ref), chan_err(fused, ref), chan_err(fused, unfused)
    print("c3h2_layer fused %s: U=%.3g fused=%.3g fused_vs_unfused=%.3g max|ref|=%.3g" % (case, u, f, fu, np.abs(ref).max()))
    assert np.isfinite(fused).all()
    assert f < bar and fu < bar, (case, f, fu, bar)


def _conv3_grid(H, W, B):
    h, w = H // 4, W // 4
    assert h % 8 == 0      # (see the module docstring: no partial tile row in the FUSE instance)
    return h, w, (h // 8) * -(-w // 16) * B


def _clean_env(monkeypatch, **env):
    for k in ("DT_C3H2", "DT_C3FUSE", "DT_H2_MINFRAMES", "DT_PIN", "DT_WINO", "DT_WINO_FUSED4", "DT_S3", "DT_S3_H2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_fused_half_empty_tile_column(monkeypatch):
    """16 frames of 64x96: conv_3 at 16x24 -- the second tile column holds 8 of 16 pixels; 64 items, one per workgroup (a workgroup's
    only item is its last: the fused tail followed by no next item)"""
    _clean_env(monkeypatch, DT_C3H2="2")
    H, W, B = 64, 96, 16
    c, layers = _detector_from(synth.synth_darknet_blob(C, seed=1234), H, W)
    h, w, items = _conv3_grid(H, W, B)
    assert w % 16 == 8 and items <= _workgroups(c)
    p2, fused, unfused = _fused_and_unfused(c, monkeypatch, dev(_frames(B, H, W, 41), c))
    _judge("64x96x16", fused.cpu().numpy(), unfused.cpu().numpy(), _ref_conv34(p2.cpu().numpy(), layers))


def test_fused_partial_columns_and_second_items(monkeypatch):
    """12 frames of 352x288 (DT_H2_MINFRAMES at its default): conv_3 at 88x72 -- 4.5 tiles per row; 660 items: some workgroups take a
    second item (the ring base moves to 1), the others end after their first"""
    _clean_env(monkeypatch, DT_C3H2="2")
    H, W, B = 352, 288, 12
    c, layers = _detector_from(synth.synth_darknet_blob(C, seed=1234), H, W)
    G = _workgroups(c)
    h, w, items = _conv3_grid(H, W, B)
    assert w % 16 == 8 and G < items < 2 * G, (items, G)
    p2, fused, unfused = _fused_and_unfused(c, monkeypatch, dev(_frames(B, H, W, 42), c))
    _judge("352x288x12", fused.cpu().numpy(), unfused.cpu().numpy(), _ref_conv34(p2.cpu().numpy(), layers))


def test_fused_ring_base_rotates(monkeypatch):
    """3 G + 64 frames of 32x64 (64 distinct ones repeated) at the DEFAULT policy: conv_3 runs at exactly one 8x16 tile per frame, item =
    frame.  Workgroups 0..63 run four items -- ring bases 0, 1, 2 and 0 again -- and every distinct frame is computed at every ring base.
    (conv_2 before it is the pooled WN = 1 instance at 2 items per frame; covered in passing, not asserted on.)"""
    _clean_env(monkeypatch)
    H, W, K = 32, 64, 64
    c, layers = _detector_from(synth.synth_darknet_blob(C, seed=1234), H, W)
    G = _workgroups(c)
    B = 3 * G + K
    h, w, items = _conv3_grid(H, W, B)
    assert (h, w) == (8, 16) and items == B
    turns = _assert_turnover(B, K, 1, G, 4)
    assert all({t % 3 for t in ts} == {0, 1, 2} and 3 in ts for ts in turns)      # sbase = turn % 3; turn 3: base 0 after a full rotation
    distinct = _frames(K, H, W, 43)
    idx = torch.arange(B, device=c.device) % K
    frames = dev(distinct, c)[idx].contiguous()
    p2, fused, unfused = _fused_and_unfused(c, monkeypatch, frames)
    assert torch.equal(p2, p2[:K][idx])      # (the reference's input is the same for every copy)
    _judge("32x64x(3G+64)", fused[:K].cpu().numpy(), unfused[:K].cpu().numpy(), _ref_conv34(p2[:K].cpu().numpy(), layers))
    same = (fused == fused[:K][idx]).flatten(1).all(1)
    assert bool(same.all()), "frames whose bits differ from their first copy: %s" % torch.nonzero(~same).flatten()[:16].tolist()


def _wave0_ratio(p2, layers):
    """smallest ratio, over the 8 x 16 tiles, of the tile's max |y| to the max |y| wave 0 holds (rows 0..3 of the tile, channels 0..63)"""
    y = np.abs(_ref_conv34(p2, layers, last=3))
    r = []
    for ty in range(0, y.shape[1], 8):
        for tx in range(0, y.shape[2], 16):
            t = y[:, ty:ty + 8, tx:tx + 16]
            r.append((t.max(axis=(1, 2, 3)) / t[:, :4, :, :64].max(axis=(1, 2, 3))).min())
    return float(min(r))


def _selection_blob(odd, seed):
    """conv_4 as a signed selection: output n = +-(conv_3 channel 2 n + odd), so that each of conv_3's 128 channels is judged on its own
    and not inside a 128-term sum (times 32: every channel's largest value then lies near or above 1, where chan_err is relative to it).
    conv_3's channels 0..63 are scaled down by 64 -- gamma AND beta, so that the folded scale and shift both carry the exact factor 2^-6
    and y there is the unscaled y / 64 -- and up again in conv_4 (exact powers of two).  The waves that hold channels 64..127 then carry the
    tile's max |y|, and wave 0 (channels 0..63, rows 0..3) sees 1/64 of what it would see unscaled: the test asserts a ratio above 16 for
    every tile, where fp16 leaves a factor below 4 of headroom over the scaled maximum -- a tile scale taken from wave 0 alone overflows."""
    rs = np.random.RandomState(seed)
    blob = synth.synth_darknet_blob(C, seed=1234).copy()
    sec = _sections(blob)
    sec[3]["gamma"][:64] *= np.float32(1.0 / 64)
    sec[3]["beta"][:64] *= np.float32(1.0 / 64)
    k4 = sec[4]["kernel"]
    k4[...] = 0.0
    for n in range(64):
        ch = 2 * n + odd
        k4[n, ch, 0, 0] = rs.choice([-1.0, 1.0]) * 32.0 * (64.0 if ch < 64 else 1.0)
    sec[4]["gamma"][:] = rs.uniform(0.5, 2.0, 64)
    sec[4]["var"][:] = rs.uniform(0.25, 4.0, 64)
    return blob


def test_fused_conv4_as_signed_selection(monkeypatch):
    _clean_env(monkeypatch, DT_C3H2="2")
    H, W, B = 64, 96, 16
    frames = _frames(B, H, W, 44)
    c = None
    for odd in (0, 1):
        blob = _selection_blob(odd, 50 + odd)
        if c is None:
            c, layers = _detector_from(blob, H, W)
        else:
            assert c.load_darknet_weights(blob) == blob.size
            layers, _ = orc.parse_darknet_blob(blob, C)
        k4 = layers[4]["kernel"][0, 0]                                # [128, 64]
        assert ((k4 != 0).sum(0) == 1).all() and sorted(np.nonzero(k4)[0].tolist()) == list(range(odd, 128, 2))
        p2, fused, unfused = _fused_and_unfused(c, monkeypatch, dev(frames, c))
        ref = _ref_conv34(p2.cpu().numpy(), layers)
        assert np.abs(ref).reshape(-1, 64).max(0).min() > 0.5      # every selected channel carries values of the bar's own scale
        # premise of the blob: in every 8 x 16 tile, max |y| over wave 0's share is more than 16 times below the tile's
        ratio = _wave0_ratio(p2.cpu().numpy(), layers)
        print("c3h2_layer selection: tile max |y| / wave 0's max |y|: min %.3g" % ratio)
        assert ratio > 16.0, ratio
        _judge("selection_%s" % ("odd" if odd else "even"), fused.cpu().numpy(), unfused.cpu().numpy(), ref, SELECTION_BAR)


def test_fused_all_zero_tiles(monkeypatch):
    """beta = mean = 0 in conv_1..conv_3 (and mean = 0 in conv_4, so that its folded bias IS beta, bit for bit): a black frame is zero up to
    conv_3's LeakyReLU, its tiles' max |y| is 0 and dt_h2_base works at its clamp.  leaky_re_lu_4 there = LeakyReLU(conv_4's bias)."""
    _clean_env(monkeypatch, DT_C3H2="2")
    H, W, B = 64, 96, 16
    black = [0, 5, 6, 15]
    blob = synth.synth_darknet_blob(C, seed=1234).copy()
    sec = _sections(blob)
    for i in (1, 2, 3):
        sec[i]["beta"][:] = 0.0
        sec[i]["mean"][:] = 0.0
    sec[4]["mean"][:] = 0.0
    c, layers = _detector_from(blob, H, W)
    frames = _frames(B, H, W, 45)
    frames[black] = 0
    p2, fused, unfused = _fused_and_unfused(c, monkeypatch, dev(frames, c))
    p2, fused, unfused = p2.cpu().numpy(), fused.cpu().numpy(), unfused.cpu().numpy()
    assert not p2[black].any() and np.abs(p2).max() > 0.1      # conv_3 reads zeros there (and its folded bias is 0): every tile's y is 0
    b4 = layers[4]["beta"].astype(np.float32)
    want = np.maximum(b4, b4 * LEAKY)
    assert np.abs(want).min() > 0
    got = fused[black].reshape(-1, 64)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), np.tile(want.view(np.uint32), (got.shape[0], 1)))
    _judge("zero_tiles", fused, unfused, _ref_conv34(p2, layers))
