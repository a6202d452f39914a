"""The tiny trackers' kernels (csrc/recurrent.hip) one by one, on the device, against the plain references of tests/tiny_units_ref.py.

1. The LSTM step, unit by unit.  One context holds the synth_tiny_weights LSTM at D = 36 (pads to 64) with dense_kernel = I, dense_bias = 0:
   O = 512 takes the fp32 MFMA head, a product with the identity is exact, so dt_tiny_sequence returns sigmoid(h) of every unit of every
   step and h = log(s / (1 - s)) in float64.  t = 0 is lstm_step0_kernel, t >= 1 the GEMV kernel reading a non-zero h_prev at stride T U;
   the stream form is the same template, its t = 0 the GEMV with the zero-select.  Track counts: one ragged group (1, 7), one full group (8),
   a full group and a ragged one (9, 13), a block less one (63), one block (64), a block and one track (65), a second block of one group (72),
   a third block (129).
   Tolerance, computed per case from the references alone: tol = 8 max|H32 - H64| + 4 floor (tiny_units_ref.lstm_case).  Measured:

       n x T     max|H32 - H64|   round-trip floor   tol        device max|h - H64|
       13 x 1    1.05e-07         3.04e-07           2.06e-06   2.68e-07
       13 x 2    1.55e-07         3.48e-07           2.63e-06   2.69e-07
       1 x 3     1.13e-07         2.84e-07           2.04e-06   2.88e-07
       7 x 3     1.51e-07         2.93e-07           2.38e-06   2.82e-07
       8 x 3     1.65e-07         2.93e-07           2.49e-06   3.40e-07
       9 x 3     1.43e-07         3.19e-07           2.42e-06   2.89e-07
       13 x 3    1.59e-07         3.25e-07           2.57e-06   3.08e-07
       63 x 3    1.73e-07         3.30e-07           2.70e-06   3.30e-07
       64 x 3    2.04e-07         3.29e-07           2.95e-06   3.09e-07
       65 x 3    1.84e-07         3.36e-07           2.82e-06   3.50e-07
       72 x 3    1.89e-07         3.37e-07           2.86e-06   3.88e-07
       129 x 3   1.96e-07         3.48e-07           2.96e-06   3.35e-07

   (device: dt_tiny_sequence on an MI355X; the stream form at 8, 9, 64, 65, 129 gives the same bits.)  The device's distance is the
   round trip's own: the step adds nothing the float32 restatement does not.  The smallest named defect (unit 511's output gate without k = 504..511) moves h by 9.0e-4 .. 3.5e-3, 360 to 1300 times the tolerance
   of its case (tests/test_tiny_units_cpu.py).
2. The pools and the concatenation through dt_tiny_features: maxima are exact, np.array_equal.
3. The heads on random dense weights against the float64 head of the float64 H: the wave-reduction kernel (O <= 8, four rows per block)
   and the MFMA head at its smallest O and at an N tail past one 256-column pad.  Tolerance per output: 8 x (orc.dense_sigmoid, float32
   sequential, against the float64 head on the same H: 3.5e-8 .. 2.3e-7) + 0.25 sum_k |Wd[k, o]| x the H tolerance of the case
   (R = 1, 5, 9 rows as 1 x 1, 1 x 5, 3 x 3 tracks x steps: 1.36e-6, 2.37e-6, 2.29e-6); 1.7e-5 .. 3.5e-5 in all.  Measured on the
   device: 1.3e-8 .. 7.7e-8 for the wave-reduction head, 9.8e-8 (O = 9) and 2.5e-7 (O = 257) for the MFMA head.
4. The heatmap helpers at hs = 1, 7, 33 (64 for the rectangle): exact, against the restatements that tests/test_tiny_units_cpu.py ties
   to the reference functions' recorded results.
"""
import functools

import numpy as np
import pytest
import torch

import mi355_dt
from oracle import oracle as orc

import tiny_units_ref as tur

pytestmark = pytest.mark.gpu

U = tur.U


def dev(a, ctx):
    return torch.from_numpy(np.array(a)).to(ctx.device)      # (a copy: the cases' arrays are read-only)


# ------------------------------------------------------------------ contexts: one with the identity head, one that is reloaded per case
@functools.lru_cache(maxsize=None)
def identity_ctx():
    tw = tur.weights()
    eye, zero = tur.identity_head()
    ctx = mi355_dt.Context()
    ctx.tiny_load(tur.D_ROWS, U, tw["kernel"], tw["recurrent"], tw["bias"], eye, zero)
    return ctx


@functools.lru_cache(maxsize=None)
def scratch_ctx():
    return mi355_dt.Context()


@functools.lru_cache(maxsize=None)
def stateless(n, T):
    """(x on the device, dt_tiny_sequence's sigmoid(h) [n,T,512]) -- computed once, never written"""
    ctx = identity_ctx()
    x = dev(tur.lstm_case(n, T).x, ctx)
    return x, ctx.tiny_sequence(x)


# ------------------------------------------------------------------ 1. the LSTM step
@pytest.mark.parametrize("n,T", tur.LSTM_CASES)
def test_lstm_step_unit_by_unit(n, T):
    case = tur.lstm_case(n, T)
    tur.check_conditions(case)
    _, s = stateless(n, T)
    assert s.shape == (n, T, U) and s.dtype == torch.float32
    tur.assert_all_close(tur.logit64(s.cpu().numpy()), case, "dt_tiny_sequence")


@pytest.mark.parametrize("n", tur.STREAM_NS)
def test_lstm_stream_step_unit_by_unit(n):
    """fresh slots scattered over a table of 2 n + 3 in descending order, chunks [1, 2]: step 0 is the GEMV with the zero-select, step 1
    reads h from the table, step 2 from the call's own rows"""
    ctx = identity_ctx()
    case = tur.lstm_case(n, 3)
    tur.check_conditions(case)
    x, whole = stateless(n, 3)
    slots = [2 * (n - 1 - i) + 1 for i in range(n)]
    assert len(set(slots)) == n and max(slots) < 2 * n + 3 and slots == sorted(slots, reverse=True)
    ctx.tiny_stream_open(2 * n + 3)
    got = torch.cat([ctx.tiny_stream_sequence(x[:, a:b].contiguous(), slots) for a, b in ((0, 1), (1, 3))], dim=1)
    tur.assert_all_close(tur.logit64(got.cpu().numpy()), case, "dt_tiny_stream_sequence")
    assert torch.equal(got, whole)


# ------------------------------------------------------------------ 2. pools and concatenation
def load_for_rows(ctx, D):
    """any weights of the right shapes: dt_tiny_features reads D alone"""
    ctx.tiny_load(D, U, np.zeros((D, 4 * U), dtype=np.float32), np.zeros((U, 4 * U), dtype=np.float32), np.zeros(4 * U, dtype=np.float32),
                  np.zeros((U, 4), dtype=np.float32), np.zeros(4, dtype=np.float32))


def check_rows(ctx, feat, det, D, pool, ref):
    n, fdim = feat.shape[0], ref.shape[1]
    assert fdim + det.shape[1] == D
    x = ctx.tiny_features(dev(feat, ctx), dev(det, ctx), D, pool).cpu().numpy()
    assert x.shape == (n, D)
    assert np.array_equal(x[:, :fdim], ref), "pooled columns: %d of %d differ" % (int((x[:, :fdim] != ref).sum()), ref.size)
    assert np.array_equal(x[:, fdim:], det), "the det columns did not land in columns %d..%d unchanged" % (fdim, D - 1)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fh,fw,C,ddim", tur.GLOBAL_CASES)
def test_global_maxpool_and_det_columns(fh, fw, C, ddim, n):
    ctx = scratch_ctx()
    D = C + ddim
    load_for_rows(ctx, D)
    rs = np.random.RandomState(C + n)
    for feat in tur.global_inputs(n, fh, fw, C, seed=100 * C + n):
        det = rs.rand(n, ddim).astype(np.float32)
        check_rows(ctx, feat, det, D, "Global", tur.global_maxpool(feat))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W,C,ddim", tur.MAX_CASES)
def test_maxpool4_flatten_and_det_columns(H, W, C, ddim, n):
    ctx = scratch_ctx()
    fdim = (H // 4) * (W // 4) * C
    load_for_rows(ctx, fdim + ddim)
    feat = tur.max_inputs(n, H, W, C, seed=H * W + n)
    det = np.random.RandomState(H + n).rand(n, ddim).astype(np.float32)
    ref = tur.maxpool4_flatten(feat)
    assert ref.shape == (n, fdim) and ref.max() < 50.0      # (the dropped rows and columns hold 100 and more)
    check_rows(ctx, feat, det, fdim + ddim, "Max", ref)


def test_global_maxpool_refuses_channels_not_a_multiple_of_4():
    ctx = scratch_ctx()
    load_for_rows(ctx, 10)
    rs = np.random.RandomState(6)
    feat, det = rs.randn(2, 3, 3, 6).astype(np.float32), rs.rand(2, 4).astype(np.float32)
    with pytest.raises(mi355_dt.NativeError):
        ctx.tiny_features(dev(feat, ctx), dev(det, ctx), 10, "Global")
    feat, det = rs.randn(2, 3, 3, 4).astype(np.float32), rs.rand(2, 6).astype(np.float32)      # the context still serves a valid call
    check_rows(ctx, feat, det, 10, "Global", tur.global_maxpool(feat))


# ------------------------------------------------------------------ 3. the heads
HEAD_CASES = [(O, R) for O in (1, 3, 8) for R in sorted(tur.HEAD_ROWS)] + [(9, 5), (257, 5)]      # wave-reduction head; MFMA head


@pytest.mark.parametrize("O,R", HEAD_CASES)
def test_dense_heads(O, R):
    n, T = tur.HEAD_ROWS[R]
    case, tw = tur.lstm_case(n, T), tur.weights()
    Wd, bd = tur.head_weights(O)
    tol, gap = tur.head_tolerance(case, Wd, bd, orc.dense_sigmoid)
    ctx = scratch_ctx()
    ctx.tiny_load(tur.D_ROWS, U, tw["kernel"], tw["recurrent"], tw["bias"], Wd, bd)
    got = ctx.tiny_sequence(dev(case.x, ctx)).cpu().numpy().astype(np.float64)
    ref = tur.dense_sigmoid64(case.H64, Wd, bd)
    assert got.shape == ref.shape == (n, T, O) and np.isfinite(got).all()
    err = np.abs(got - ref).reshape(-1, O).max(axis=0)
    print("O=%d R=%d: max|out - ref| %.3g; float32 head vs float64 %.3g, tolerance %.3g .. %.3g" % (O, R, err.max(), gap, tol.min(), tol.max()))
    assert (err <= tol).all(), "outputs %s off by %s (tolerance %s)" % (np.nonzero(err > tol)[0][:8], err[err > tol][:8], tol[err > tol][:8])


# ------------------------------------------------------------------ 4. the heatmap helpers
@pytest.mark.parametrize("hs", tur.HEAT_SIZES)
def test_heatmaps_from_boxes(hs):
    ctx = scratch_ctx()
    boxes = tur.heat_boxes()
    ref = np.stack([tur.heatmap_feat(*b, hs=hs) for b in boxes])
    got = ctx.heatmap_from_xywh64(dev(boxes, ctx), hs).cpu().numpy()
    assert got.shape == ref.shape == (len(boxes), hs * hs)
    assert np.array_equal(got, ref), "boxes %s" % np.nonzero((got != ref).any(axis=1))[0]
    c4, corners = tur.centre_boxes()
    ref = np.stack([tur.heatmap_feat(*b, hs=hs) for b in corners])
    got = ctx.heatmap_from_boxes(dev(c4, ctx), hs).cpu().numpy()
    assert np.array_equal(got, ref), "centre-format boxes %s" % np.nonzero((got != ref).any(axis=1))[0]


@pytest.mark.parametrize("hs", tur.RECT_SIZES)
def test_rect_from_heatmap(hs):
    ctx = scratch_ctx()
    maps = tur.rect_maps(hs)
    ref = np.array([tur.rect_of_heatmap(m, tur.THRESH, hs) for m in maps], dtype=np.int32)
    assert ref[0].tolist() == [hs, hs, -1, -1] and ref[3, 2] >= 0 and ref[4].tolist() == [hs, hs, -1, -1]      # >= counts, one ulp below does not
    got = ctx.rect_from_heatmap(dev(maps, ctx), hs, tur.THRESH)
    assert got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), ref), (got.cpu().numpy().tolist(), ref.tolist())
