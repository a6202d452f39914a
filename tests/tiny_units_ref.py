"""Plain numpy restatements of the tiny trackers' pieces (csrc/recurrent.hip), for the tests: the LSTM recurrence in any dtype, the two
pools, the Dense head, the two heatmap helpers; the table of LSTM cases with the tolerance each one earns; and a table of named defects.

The LSTM (Keras 2.x, implementation=2): z = x.W + b + h.R, gate order i, f, c, o; i, f, o = hard_sigmoid(z) = clip(0.2 z + 0.5, 0, 1),
g = tanh(z_c); c' = f c + i g; h' = o tanh(c').  The float64 run is the reference; the float32 run exists only to size the tolerance.

Reading h out of the library: with dense_kernel = I (512 x 512) and dense_bias = 0 the head is the fp32 MFMA GEMM (exact fp32 products,
and a row of the identity has one non-zero term) with 1 / (1 + expf(-z)), so dt_tiny_sequence returns sigmoid(h) for every unit of every
step and h = log(s / (1 - s)) in float64.  |h| <= 1 (h = o tanh c), so s lies in [0.26, 0.74] and the round trip costs a few 1e-7.

The tolerance of a case is computed from the references alone:  tol = 8 max|H32 - H64| + 4 floor,  floor = max|logit64(sigmoid32(H64)) - H64|.
The margin of 8: the kernel's summation order (eight-term FMA chains per lane, then a tree) and the GEMM's differ from numpy's, and all of
them obey the same gamma_n sum|terms| bound.  Test infrastructure only.
"""
import functools

import numpy as np

from utility import synth

U = 512
D_ROWS = 36                 # 32 pooled channels + a 4-box: pads to 64 in the projection, so pad columns are in play
LSTM_NS = (1, 7, 8, 9, 13, 63, 64, 65, 72, 129)
LSTM_CASES = tuple([(13, 1), (13, 2)] + [(n, 3) for n in LSTM_NS])      # (n tracks, T steps)
STREAM_NS = (8, 9, 64, 65, 129)
HEAD_ROWS = {1: (1, 1), 5: (1, 5), 9: (3, 3)}      # R = n T rows of the head tests -> (n, T)


# ------------------------------------------------------------------ the recurrence
def hard_sigmoid(z):
    t = z.dtype.type
    return np.clip(t(0.2) * z + t(0.5), t(0), t(1))


def lstm_sequence(x, kernel, recurrent, bias, dtype=np.float64, mutate=None, pre=False):
    """x [n,T,D] -> H [n,T,U] (pre: and the pre-activations Z [n,T,4U]).  mutate(rec, h, R, t) -> rec stands in for a defect of the
    recurrent term rec = h.R [n,4U] of step t (h [n,U] is the state it was formed from)."""
    x, W, R, b = (np.asarray(a, dtype=dtype) for a in (x, kernel, recurrent, bias))
    n, T, _ = x.shape
    units = R.shape[0]
    h = np.zeros((n, units), dtype=dtype)
    c = np.zeros_like(h)
    H = np.empty((n, T, units), dtype=dtype)
    Z = np.empty((n, T, 4 * units), dtype=dtype)
    for t in range(T):
        rec = h @ R
        if mutate is not None:
            rec = mutate(rec.copy(), h, R, t)
        z = (x[:, t] @ W + b) + rec
        zi, zf, zc, zo = (z[:, g * units:(g + 1) * units] for g in range(4))
        c = hard_sigmoid(zf) * c + hard_sigmoid(zi) * np.tanh(zc)
        h = hard_sigmoid(zo) * np.tanh(c)
        H[:, t], Z[:, t] = h, z
    return (H, Z) if pre else H


# ------------------------------------------------------------------ named defects of the recurrent term
SLICE = slice(504, 512)      # lane 63's k-slice of the GEMV


def _m_unit511_o_loses_lane63(rec, h, R, t):
    rec[:, 3 * U + 511] -= h[:, SLICE] @ R[SLICE, 3 * U + 511]
    return rec


def _m_cell_gate_loses_lane63(rec, h, R, t):
    rec[:, 2 * U:3 * U] -= h[:, SLICE] @ R[SLICE, 2 * U:3 * U]
    return rec


def _m_tracks_8_9_swap_high_units(rec, h, R, t):
    for g in range(4):
        cols = slice(g * U + 448, (g + 1) * U)
        rec[[8, 9], cols] = rec[[9, 8], cols]
    return rec


def _m_ragged_tail_takes_its_neighbour(rec, h, R, t):
    rec[-1] = rec[-2]
    return rec


def _m_unit0_f_o_swap(rec, h, R, t):
    rec[:, [U, 3 * U]] = rec[:, [3 * U, U]]
    return rec


# name -> (defect, the track counts it applies to)
MUTATIONS = {
    "unit511_o_loses_lane63": (_m_unit511_o_loses_lane63, lambda n: True),
    "cell_gate_loses_lane63": (_m_cell_gate_loses_lane63, lambda n: True),
    "tracks_8_9_swap_high_units": (_m_tracks_8_9_swap_high_units, lambda n: n >= 10),
    "ragged_tail_takes_its_neighbour": (_m_ragged_tail_takes_its_neighbour, lambda n: n % 8 > 1),      # a ragged group with a track before the last
    "unit0_f_o_swap": (_m_unit0_f_o_swap, lambda n: True),
}


# ------------------------------------------------------------------ read-out through the identity head
def identity_head():
    return np.eye(U, dtype=np.float32), np.zeros(U, dtype=np.float32)


def logit64(s):
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(s / (1.0 - s))


def roundtrip_floor(H64):
    """what sigmoid in float32 followed by the float64 logit costs on these values"""
    h = H64.astype(np.float32)
    s = np.float32(1) / (np.float32(1) + np.exp(-h))
    assert s.dtype == np.float32
    return float(np.abs(logit64(s) - H64).max())


# ------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def weights():
    """the synth_tiny_weights LSTM at D = 36 (read-only)"""
    tw = synth.synth_tiny_weights(D_ROWS - 4)
    assert tw["kernel"].shape == (D_ROWS, 4 * U)
    for a in tw.values():
        a.setflags(write=False)
    return tw


def inside_fraction(Z):
    """share of the i, f and o pre-activations strictly inside the hard sigmoid's slope (-2.5, 2.5)"""
    z = np.concatenate([Z[..., :2 * U], Z[..., 3 * U:]], axis=-1)
    return float((np.abs(z) < 2.5).mean())


def min_track_distance(H):
    """min over pairs of tracks of max over (step, unit) of |H_a - H_b|"""
    n = H.shape[0]
    best = np.inf
    for a in range(n - 1):
        best = min(best, float(np.abs(H[a + 1:] - H[a]).reshape(n - 1 - a, -1).max(axis=1).min()))
    return best


class Case(object):
    pass


@functools.lru_cache(maxsize=None)
def lstm_case(n, T):
    """rows x [n,T,36] float32 straight from a seeded generator, scaled down until at least 90 % of the reference's i, f and o
    pre-activations lie inside the slope; H64, H32, the round-trip floor and the tolerance.  Computed once, read-only."""
    tw = weights()
    base = np.random.RandomState(4000 + 16 * n + T).randn(n, T, D_ROWS)
    for scale in (4.0, 2.0, 1.0, 0.5):
        x = (base * scale).astype(np.float32)
        H64, Z = lstm_sequence(x, tw["kernel"], tw["recurrent"], tw["bias"], np.float64, pre=True)
        if inside_fraction(Z) >= 0.9:
            break
    c = Case()
    c.n, c.T, c.scale, c.x, c.H64, c.Z = n, T, scale, x, H64, Z
    c.H32 = lstm_sequence(x, tw["kernel"], tw["recurrent"], tw["bias"], np.float32)
    assert c.H32.dtype == np.float32
    c.gap = float(np.abs(c.H32.astype(np.float64) - H64).max())
    c.floor = roundtrip_floor(H64)
    c.tol = 8.0 * c.gap + 4.0 * c.floor
    for a in (c.x, c.H64, c.H32, c.Z):
        a.setflags(write=False)
    return c


def mutated(case, name):
    tw = weights()
    return lstm_sequence(case.x, tw["kernel"], tw["recurrent"], tw["bias"], np.float64, mutate=MUTATIONS[name][0])


def check_conditions(case):
    """the conditions on a case's inputs -- on the reference alone"""
    assert inside_fraction(case.Z) >= 0.9, "saturated gates hide errors in z: %.3f inside" % inside_fraction(case.Z)
    assert 0.0 < case.tol < 1e-4, case.tol
    if case.n > 1:
        d = min_track_distance(case.H64)
        assert d >= 100.0 * case.tol, "two tracks are %.3g apart at a tolerance of %.3g: a permutation could pass" % (d, case.tol)


def assert_all_close(got, case, what):
    """every track, step and unit of got within the case's tolerance of H64"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == case.H64.shape, (got.shape, case.H64.shape)
    assert np.isfinite(got).all(), "%s: %d values are not finite" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - case.H64)
    worst = np.unravel_index(int(err.argmax()), err.shape)
    print("%s n=%d T=%d: max|h - H64| %.3g at (track, step, unit) %s; tol %.3g (gap %.3g, floor %.3g)"
          % (what, case.n, case.T, err.max(), worst, case.tol, case.gap, case.floor))
    assert err.max() <= case.tol, "%s: %d of %d values off by more than %.3g, worst %.3g at (track, step, unit) %s" % (
        what, int((err > case.tol).sum()), err.size, case.tol, err.max(), worst)


# ------------------------------------------------------------------ the head
def dense_sigmoid64(H, Wd, bd):
    z = np.asarray(H, dtype=np.float64) @ np.asarray(Wd, dtype=np.float64) + np.asarray(bd, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(-z))


def head_weights(O):
    rs = np.random.RandomState(7000 + O)
    return rs.uniform(-0.2, 0.2, (U, O)).astype(np.float32), (rs.randn(O) * 0.1).astype(np.float32)


def head_tolerance(case, Wd, bd, dense_sigmoid32):
    """per output: 8 x (a float32 sequential head against the float64 head on the same H) + the case's H tolerance pushed through the
    head -- the sigmoid's slope is at most 0.25, so an error e in every unit moves output o by at most 0.25 e sum_k |Wd[k, o]|"""
    H = case.H64.reshape(-1, U)
    ref = dense_sigmoid64(H.astype(np.float32), Wd, bd)
    gap = float(np.abs(dense_sigmoid32(H.astype(np.float32), Wd, bd).astype(np.float64) - ref).max())
    return 8.0 * gap + 0.25 * np.abs(Wd.astype(np.float64)).sum(axis=0) * case.tol, gap


# ------------------------------------------------------------------ the pools
def global_maxpool(feat):
    """[n,fh,fw,C] -> [n,C]"""
    return feat.reshape(feat.shape[0], -1, feat.shape[3]).max(axis=1)


def maxpool4_flatten(feat):
    """MaxPooling2D((4,4)) + Flatten: [n,H,W,C] -> [n,(H//4)(W//4)C] in (h4, w4, c) order; rows and columns past a multiple of 4 are dropped"""
    n, H, W, C = feat.shape
    H4, W4 = H // 4, W // 4
    return feat[:, :4 * H4, :4 * W4].reshape(n, H4, 4, W4, 4, C).max(axis=(2, 4)).reshape(n, H4 * W4 * C)


GLOBAL_CASES = ((1, 1, 4, 4), (1, 2, 8, 5), (1, 3, 260, 4), (2, 2, 256, 4), (1, 5, 252, 4), (13, 13, 512, 4), (1, 7, 1028, 1024),
                (1, 1, 4, 5))      # (fh, fw, C, ddim); the last: D = 9, an odd stride next to the smallest D the load takes (8, the first)
MAX_CASES = ((4, 4, 1, 7), (13, 13, 32, 4), (8, 12, 5, 4), (7, 9, 3, 4), (16, 4, 2, 4))      # (H, W, C, ddim)


def global_inputs(n, fh, fw, C, seed):
    """two maps [n,fh,fw,C]: negative everywhere; and one whose channel c peaks at pixel c mod HW (every wavefront's share of the pixels,
    the last pixel among them, decides some channel)"""
    rs = np.random.RandomState(seed)
    neg = -(rs.rand(n, fh, fw, C) + 0.5).astype(np.float32)
    peak = rs.randn(n, fh * fw, C).astype(np.float32)
    c = np.arange(C)
    peak[:, c % (fh * fw), c] = 10.0 + rs.rand(n, C).astype(np.float32)
    return neg, peak.reshape(n, fh, fw, C)


def max_inputs(n, H, W, C, seed):
    """[n,H,W,C] whose rows and columns past a multiple of 4 hold the largest values of the map"""
    rs = np.random.RandomState(seed)
    f = rs.randn(n, H, W, C).astype(np.float32)
    f[:, 4 * (H // 4):] += 100.0
    f[:, :, 4 * (W // 4):] += 100.0
    return f


# ------------------------------------------------------------------ the heatmap helpers
def heatmap_feat(det_x, det_y, det_w, det_h, hs):
    """the data generator's box -> 0/1 map rule: the corner and the size are scaled by hs and truncated toward zero, and rows
    sy .. sy + sh, columns sx .. sx + sw are set by a Python slice -- negative bounds count from the end, as slices do."""
    sx, sy, sh, sw = int(det_x * hs), int(det_y * hs), int(det_h * hs), int(det_w * hs)
    rows = np.zeros(hs, dtype=bool)
    cols = np.zeros(hs, dtype=bool)
    rows[list(range(*slice(sy, sy + sh + 1).indices(hs)))] = True
    cols[list(range(*slice(sx, sx + sw + 1).indices(hs)))] = True
    return np.outer(rows, cols).astype(np.float32).reshape(-1)


def rect_of_heatmap(heat, thresh, hs):
    """bounding (x1, y1, x2, y2) of the cells >= thresh, compared in float64; (hs, hs, -1, -1) when there is none"""
    i, j = np.nonzero(np.asarray(heat, dtype=np.float64).reshape(hs, hs) >= float(thresh))
    if i.size == 0:
        return hs, hs, -1, -1
    return int(j.min()), int(i.min()), int(j.max()), int(i.max())


HEAT_SIZES = (1, 7, 33)
RECT_SIZES = (1, 7, 33, 64)
THRESH = 0.75                # a float32 number, so the kernel's float threshold and the reference's double agree


def heat_boxes():
    """(x, y, w, h) float64, corner format: negative corners (from-the-end slices, with the stop negative too), a corner beyond -hs,
    a box past the far edge, one that starts past it, w = h = 0, boxes that cover everything, and two ordinary ones"""
    return np.array([[-0.2, -0.3, 0.5, 0.6], [-0.9, -0.8, 0.3, 0.2], [-0.45, 0.1, 0.3, 0.3], [-1.5, -2.2, 0.9, 3.0], [-1.25, -1.25, 0.1, 0.1],
                     [0.8, 0.7, 0.6, 0.9], [1.3, 1.2, 0.2, 0.2], [0.4, 0.6, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0],
                     [-0.1, -0.1, 5.0, 5.0], [0.3, 0.2, 0.25, 0.4], [0.52, 0.13, 0.31, 0.77]], dtype=np.float64)


def centre_boxes():
    """the same boxes in the float32 centre format dt_heatmap_from_boxes takes; the corner they stand for is formed in float64 from the
    float32 numbers, as the data generator does: (cx - w / 2.0, cy - h / 2.0, w, h)"""
    b = heat_boxes()
    c4 = np.stack([b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2, b[:, 2], b[:, 3]], axis=1).astype(np.float32)
    c = c4.astype(np.float64)
    return c4, np.stack([c[:, 0] - c[:, 2] / 2.0, c[:, 1] - c[:, 3] / 2.0, c[:, 2], c[:, 3]], axis=1)


def rect_maps(hs):
    """[7, hs*hs] float32: empty; only the last cell; only cell 0; one cell exactly at the threshold (counts: the rule is >=); the same
    cell one ulp below it (does not); both among lower values; a random soft map"""
    t = np.float32(THRESH)
    below = np.nextafter(t, np.float32(0))
    assert float(t) == THRESH and below < t
    cells = hs * hs
    mid = (hs // 2) * hs + (2 * hs) // 3
    m = np.zeros((7, cells), dtype=np.float32)
    m[1, cells - 1] = 1.0
    m[2, 0] = 1.0
    m[3, mid] = t
    m[4, mid] = below
    m[5] = 0.5
    m[5, mid] = t
    m[5, (mid + 1) % cells] = below
    m[6] = np.random.RandomState(50 + hs).rand(cells).astype(np.float32)
    return m
