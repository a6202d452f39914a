"""Helpers of tests/test_gpu_conv1_edges.py and tests/test_conv1_cases_cpu.py (no GPU): the launcher's rule of conv_1's direct kernels
(csrc/conv1.hip: plan_conv1) and the walk of a workgroup along x restated in numpy, integer / float64 references of the fused layer
(x/255, 3x3 'same' convolution on RGB, bias, LeakyReLU, 2x2 max), an emulation of the three-term bf16 split with its two product orders, operand
families with an exact or tightly bounded expected result, and the case table.

The layer: frames [B,H,W,3] uint8 (normalised by /255 inside) or float32 (already normalised), w [27,32] with row k = 9 ky + 3 kx + ci, bias [32],
out [B,H/2,W/2,32].  Four kernel instances (mi355_dt.h: DT_C1_*): the fp32 MFMA kernel ("mfma"), the split kernel on uint8 frames with whole
tiles only ("full": H and W multiples of 16) or with guarded stores ("u8"), and the split kernel on float32 frames ("f32").

Operand families:
  P   position codes.  float32 frames: DISTINCT integers below 2^24, randomly permuted over (b, y, x, c); uint8 frames: random bytes.  One-hot
      weights: channel n copies tap n % 27, sign - for odd n (x 255 for uint8 frames, so that w / 255 = +-1), bias 0.  Every output is one input
      value (or its negative, or a 0 of the padding) picked by a 2x2 max: expected bit for bit, and a wrong float32 value names the pixel it is.
  I   integers.  uint8 split instances: bytes (the table's extremes on the image border) against w = 255 q, q an integer in [-4, 4] -- w / 255 is
      exact and has one bf16 term; float32 frames: x in [0, 1023] against w in [-511, 511], at most 10 significant bits each, two bf16 terms each,
      all four partial products of a pair among the six the kernel forms.  Integer bias.  Every partial sum in any order is an integer below 2^24
      (sum_bound): expected bit for bit.  `Ib` is the same with weights <= 0 (the centre tap < 0), operands >= 1 and a bias so large that
      every output is positive and strictly below the bias -- the value a window of padding alone evaluates to.
  T   single products with full significands: one-hot weights with 24-bit significands against 24-bit activations (float32 frames) or bytes
      (uint8 frames), bias 0, slope 1.  Bar t_bar on |got - ref64| / |ref64|.  `Tp`: the weights are powers of two -- exact on the fp32 MFMA kernel.
  D   dense, production-like: bytes, normal weights, bias, slope 0.1; float32 frames get float32(b / 255).  Bar d_bar1 on
      |got - ref64| / (sum |a||w| + |b|) against float64 of (b / 255) w.

The 2x2 max and the bars.  An output is the maximum of four activated pre-activations.  |max_i a'_i - max_i a_i| <= max_i |a'_i - a_i|, so family
D's scale of a pooled output is the largest scale in its window.  For family T (slope 1, bias 0) each a_i is one product with relative error at
most eps; if the kernel's maximum sits at another index j than the reference's i*, a'_j >= a'_i* and a_j <= a_i* confine a_j to within
2 eps |a_i*| of a_i*: the pooled value keeps the relative bar to second order in eps (2^-21 against a measured 2^-23)."""
import numpy as np

import conv_igemm_cases as cc

SENTINEL32 = cc.SENTINEL32
C1_TPW = 26                 # conv1.hip: most tiles a workgroup walks
C1_PF = 2                   # conv1.hip: tiles of frame loads in flight (register sets rawA, rawB)
MFMA, FULL, U8, F32 = "mfma", "full", "u8", "f32"
INSTANCE_CODE = {MFMA: 0, FULL: 1, U8: 2, F32: 3}      # mi355_dt.h: DT_C1_MFMA_F32, DT_C1_S3_U8_FULL, DT_C1_S3_U8, DT_C1_S3_F32
INSTANCES = (MFMA, FULL, U8, F32)


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- the launcher's rule
def plan(B, H, W, dtype, align=0, split=1, tpw=0, slope=0.1):
    """plan_conv1 restated: None for what the launcher refuses, else the instance, the tiles a workgroup walks, the grid and fills-amax.
    dtype "u8" / "f32"; align: the frames' byte address modulo 4; split: the three-term tables are passed; tpw: 0 = the rule"""
    if H <= 0 or W <= 0 or H % 2 or W % 2 or B <= 0 or B > 65535 or not slope >= 0 or tpw < 0 or tpw > C1_TPW:
        return None
    H2, W2 = H // 2, W // 2
    rows, ntx = B * _cdiv(H2, 8), _cdiv(W2, 8)
    t = C1_TPW
    while t > 1 and rows * _cdiv(ntx, t) < 2048:
        t = (t + 1) // 2
    if tpw:
        t = tpw
    if split and (dtype != "u8" or (W % 4 == 0 and align % 4 == 0)):
        inst = F32 if dtype != "u8" else (FULL if H % 16 == 0 and W % 16 == 0 else U8)
    else:
        inst = MFMA
    return {"instance": INSTANCE_CODE[inst], "tpw": t, "grid_x": _cdiv(ntx, t), "grid_y": _cdiv(H2, 8), "grid_z": B, "fills_amax": int(inst != MFMA)}


def walks(ntx, tpw, inst):
    """per workgroup of a tile row: the tiles it walks -- (bx, position, register set, loop, the tile whose loads it requests or None) -- as the
    instance's loop runs them.  full: the pair loop ("pair") and its odd tail ("tail"), every tile requests min(bx + 2, last) -- a clamped request
    re-reads the last tile; u8 / f32: the guarded loop, a request only while bx + 2 is in the walk; mfma: one register set, one tile ahead."""
    out = []
    for wg in range(_cdiv(ntx, tpw)):
        first, last = wg * tpw, min(wg * tpw + tpw, ntx)      # [first, last)
        n = last - first
        tiles = []
        for pos in range(n):
            bx = first + pos
            if inst == MFMA:
                tiles.append(dict(bx=bx, pos=pos, set="A", loop="mfma", request=bx + 1 if bx + 1 < last else None))
            elif inst == FULL:
                tiles.append(dict(bx=bx, pos=pos, set="AB"[pos & 1], loop="tail" if (n & 1 and pos == n - 1) else "pair", request=min(bx + C1_PF, last - 1)))
            else:
                tiles.append(dict(bx=bx, pos=pos, set="AB"[pos & 1], loop="guarded", request=bx + C1_PF if bx + C1_PF < last else None))
        out.append(dict(wg=wg, tiles=tiles, kinds=walk_kinds(n, tpw)))
    return out


WALK_KINDS = ("single", "pair", "odd", "short")


def walk_kinds(n, tpw):
    """what a walk of n tiles under tpw is: a single tile (both prefetches clamp to it / none is issued), whole pairs, an odd tail behind at least
    one pair, and -- besides -- shorter than tpw (the last workgroup of a row)"""
    k = {"single" if n == 1 else ("odd" if n & 1 else "pair")}
    if n < tpw:
        k.add("short")
    return k


def locate(k, b, oy, ox, n):
    """where output (frame b, pooled row oy, pooled column ox, channel n) is computed: tile, workgroup, position in the walk, register set, loop,
    wave and lane"""
    p = k["want"]
    bx, by = ox // 8, oy // 8
    wg = bx // p["tpw"]
    t = walks(_cdiv(k["W"] // 2, 8), p["tpw"], k["inst"])[wg]["tiles"][bx - wg * p["tpw"]]
    h, j = (ox % 8) & 1, (ox % 8) >> 1
    return dict(frame=b, tile=(by, bx), workgroup=(wg, by, b), position=t["pos"], set=t["set"], loop=t["loop"], request=t["request"],
                wave=(oy % 8) // 2, group=oy % 2, lane=32 * h + n, window=h + 2 * j)


# ---------------------------------------------------------------------------------------------------------------- references
def patches(x):
    """[B,H,W,3] -> [B,H,W,27], k = 9 ky + 3 kx + ci, zero 'same' padding"""
    B, H, W, _ = x.shape
    xp = np.zeros((B, H + 2, W + 2, 3), x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    return np.concatenate([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], axis=3)


def preact(x, w):
    """the convolution of exact operands x [B,H,W,3] and w [27,32]: int64 when both are integers, float64 otherwise.  (Integer operands beyond
    2^24 multiply-adds go through float64 BLAS, every sum asserted below 2^53 and therefore exact, and come back as int64.)"""
    x, w = np.asarray(x), np.asarray(w)
    integer = bool(np.all(x == np.rint(x)) and np.all(w == np.rint(w)))
    if integer and x.size * 9 * 32 <= (1 << 24):
        return patches(x.astype(np.int64)) @ w.astype(np.int64)
    z = patches(x.astype(np.float64)) @ w.astype(np.float64)
    if integer:
        assert np.abs(x).max() * np.abs(w).sum(axis=0).max() < 2.0 ** 53
        return np.rint(z).astype(np.int64)
    return z


def preact_abs(x, w, bias):
    return patches(np.abs(np.asarray(x, np.float64))) @ np.abs(np.asarray(w, np.float64)) + np.abs(np.asarray(bias, np.float64))


def layer32(z, bias, slope):
    """the epilogue on an exact pre-activation: conv_igemm_cases.act32 (one float32 add, one float32 multiply), then the 2x2 max"""
    return cc.maxpool2(cc.act32(z, bias, slope))


def layer64(z, bias, slope):
    v = np.asarray(z, np.float64) + np.asarray(bias, np.float64)
    return cc.maxpool2(np.where(v > 0, v, v * np.float64(np.float32(slope))))


def t_bar():
    """family T: conv_igemm_cases.d_bar(1, 1) = 2^-21"""
    return cc.d_bar(1, 1)


def d_bar1():
    """family D: d_bar's derivation for K = 27 with two more roundings per product (the split; x / 255 or w / 255): 2 (27 + 2 + 3) 2^-24 = 2^-18"""
    return 2.0 * (27 + 2 + 3) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the split, emulated
def bf16_rne(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """x = x1 + x2 + x3 as conv1_s3_kernel's staging and wino_s3_split_host form them: three roundings to nearest even, exact differences"""
    x = np.asarray(x, dtype=np.float32)
    x1 = bf16_rne(x)
    r1 = (x - x1).astype(np.float32)
    x2 = bf16_rne(r1)
    return x1, x2, bf16_rne((r1 - x2).astype(np.float32))


U8_ORDER = ((0, 2), (0, 1), (0, 0))                                  # (activation term, weight term): x w'3, x w'2, x w'1
F32_ORDER = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))        # x3 w1, x2 w2, x1 w3, x2 w1, x1 w2, x1 w1


def emulate_preact(frames, w, drop=None):
    """float32 accumulators [B,H,W,32] as the split kernels form them: per product term, the two k-blocks (k 0..15, 16..26) one after the other,
    each the exact sum of its bf16 x bf16 products added into the float32 accumulator with one rounding (the model of tests/test_split_arith.py).
    uint8 frames: the bytes against the three terms of float32(float64(w) / 255); float32 frames: three terms each, six products.
    drop: index into the product order of one product to leave out."""
    if frames.dtype == np.uint8:
        xt = (patches(frames.astype(np.float64)),)
        wt = split3((np.asarray(w, np.float64) / 255.0).astype(np.float32))
        order = U8_ORDER
    else:
        xt = tuple(patches(t.astype(np.float64)) for t in split3(frames))
        wt = split3(w)
        order = F32_ORDER
    acc = np.zeros(xt[0].shape[:3] + (32,), np.float32)
    for i, (ta, tb) in enumerate(order):
        if i == drop:
            continue
        for ks in (slice(0, 16), slice(16, 27)):
            acc = (acc.astype(np.float64) + xt[ta][..., ks] @ wt[tb][ks].astype(np.float64)).astype(np.float32)
    return acc


def emulate_layer(frames, w, bias, slope, drop=None):
    """the kernel's epilogue on the emulated accumulators: 2x2 max first, then one float32 add and one float32 multiply"""
    mx = cc.maxpool2(emulate_preact(frames, w, drop))
    v = (mx + np.asarray(bias, np.float32)).astype(np.float32)
    return np.where(v > 0, v, v * np.float32(slope)).astype(np.float32)


def lut255():
    """the context's table: float32(float64(i) / 255)"""
    return (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- operands
def onehot(rs, values):
    """w [27,32]: channel n copies tap n % 27 with weight values[n], sign - for odd n"""
    w = np.zeros((27, 32), np.float64)
    n = np.arange(32)
    w[n % 27, n] = np.where(n & 1, -1.0, 1.0) * values
    return w


def _terms_rel(v):
    """|v2| / |v| and |v3| / |v| of the three-term split of float32 v"""
    _, v2, v3 = split3(v)
    a = np.abs(v.astype(np.float64))
    return np.abs(v2.astype(np.float64)) / a, np.abs(v3.astype(np.float64)) / a


def _mant24(rs, n, as_weight_of_u8=False, emin=-6, emax=6):
    """n positive float32 values with full 24-bit significands over the binades emin..emax, drawn at random and KEPT only where both lower bf16
    terms are large enough that dropping any one partial product shows: |v3| >= 8 x 2^-24 |v| and |v2| >= 2^-10 |v| (about two draws in three).
    Value 0 is replaced by a draw whose third term is nearly as large as one can be (|v3| >= 126 x 2^-24 |v|: a significand just above 1 that
    ends in half a unit of the second term), value 1 by one whose second term is (|v2| >= 0.97 x 2^-8 |v|).  as_weight_of_u8: the properties are
    those of float32(float64(v) / 255), the number the uint8 form splits."""
    def draw(m):
        s = rs.randint(1 << 23, 1 << 24, m).astype(np.float64) * 2.0 ** -23
        v = (s * np.exp2(rs.randint(emin, emax + 1, m))).astype(np.float32)
        return v, _terms_rel((v.astype(np.float64) / 255.0).astype(np.float32) if as_weight_of_u8 else v)
    v, (r2, r3) = draw(4 * n + 64)
    out = v[(r3 >= 8 * 2.0 ** -24) & (r2 >= 2.0 ** -10)][:n].copy()
    assert len(out) == n
    v, (r2, r3) = draw(1 << 20)
    out[0] = v[r3 >= 126 * 2.0 ** -24][0]
    out[1] = v[(r2 >= 0.97 * 2.0 ** -8) & (r3 >= 8 * 2.0 ** -24)][0]
    return out


def _bytes(rs, B, H, W, lo=0):
    f = rs.randint(lo, 256, (B, H, W, 3)).astype(np.uint8)
    if lo == 0:      # extremes of the x/255 table on the image border, as the detector-level test places them
        f[0, :2, :5] = 255
        f[0, -1, -3:] = 0
    return f


def operands(k):
    """dict(frames [B,H,W,3] uint8 / float32, w [27,32] float32, bias [32] float32: what the kernel is handed;
            x, wx: the EXACT operands of the reference -- integers for P / I / Ib, float64 otherwise -- with preact(x, wx) the pre-activation)"""
    rs = np.random.RandomState(k["seed"])
    B, H, W, fam, u8 = k["B"], k["H"], k["W"], k["fam"], k["dtype"] == "u8"
    bias = np.zeros(32)
    if fam == "P":
        if u8:
            frames = _bytes(rs, B, H, W)
            wx = onehot(rs, 1.0)
            w = 255.0 * wx
        else:
            n = B * H * W * 3
            step = ((1 << 24) - 2) // n
            assert step >= 1
            frames = (1 + rs.permutation(n).astype(np.int64) * step + rs.randint(0, step, n)).reshape(B, H, W, 3).astype(np.float32)
            w = wx = onehot(rs, 1.0)
        x = frames.astype(np.int64)
    elif fam in ("I", "Ib"):
        neg = fam == "Ib"
        if u8:
            frames = _bytes(rs, B, H, W, lo=1 if neg else 0)
            wx = rs.randint(-4, 1 if neg else 5, (27, 32))
            w = 255.0 * wx
        else:
            frames = rs.randint(1 if neg else 0, 1024, (B, H, W, 3)).astype(np.float32)
            w = wx = rs.randint(-255, 1, (27, 32)) if neg else rs.randint(-511, 512, (27, 32))
        if neg:
            wx[12:15] = np.minimum(wx[12:15], -1)      # the centre tap: every window with one pixel inside the image is strictly below the bias
            w = 255.0 * wx if u8 else wx
            bias = (30000 if u8 else 8000000) + np.arange(32) * 3.0      # above 27 x 255 x 4 / 27 x 1023 x 255: every output is positive
        else:
            bias = rs.randint(-2000, 2001, 32) if u8 else rs.randint(-100000, 100001, 32)
        x = frames.astype(np.int64)
    elif fam in ("T", "Tp"):
        sh = (B, H, W, 3)
        mag = np.exp2(rs.randint(-6, 7, 32)) if fam == "Tp" else rs.permutation(_mant24(rs, 32, as_weight_of_u8=u8)).astype(np.float64)
        w = wx = onehot(rs, mag)
        if u8:
            frames = _bytes(rs, B, H, W)
            x = frames.astype(np.float64) / 255.0
        else:
            frames = (rs.permutation(_mant24(rs, B * H * W * 3)).reshape(sh) * np.where(rs.randint(0, 2, sh), -1.0, 1.0)).astype(np.float32)
            x = frames.astype(np.float64)
    elif fam == "D":
        b = _bytes(rs, B, H, W)
        x = b.astype(np.float64) / 255.0
        frames = b if u8 else x.astype(np.float32)
        w = wx = (rs.randn(27, 32) * 0.4).astype(np.float32).astype(np.float64)
        bias = rs.randn(32).astype(np.float32)
    else:
        raise KeyError(fam)
    return dict(frames=np.ascontiguousarray(frames), w=np.ascontiguousarray(w, dtype=np.float32), bias=np.ascontiguousarray(bias, dtype=np.float32),
                x=x, wx=np.asarray(wx))


def sum_bound(k, o):
    """the largest |partial sum| any order of any term split can reach in an exact-family case, bias included: the bf16 terms of an operand sum to
    it with |x1| + |x2| + |x3| <= (1 + 2^-7) |x|"""
    f = (1.0 + 2.0 ** -7) ** 2
    return float((f * preact_abs(o["x"], o["wx"], 0 * o["bias"]) + np.abs(o["bias"].astype(np.float64))).max())


def expected_exact(k, o):
    """P / I / Ib: the layer on the exact integer pre-activation.  Tp: float32(table[b]) 2^e (uint8 frames) or x 2^e, exactly."""
    if k["fam"] == "Tp":
        x = lut255()[o["frames"]].astype(np.float64) if k["dtype"] == "u8" else o["frames"].astype(np.float64)
        return layer32(preact(x, o["wx"]), o["bias"], k["slope"])      # (one product per output: float64 holds it exactly, float32 too)
    return layer32(preact(o["x"], o["wx"]), o["bias"], k["slope"])


# ---------------------------------------------------------------------------------------------------------------- the case table
CASES = {}
_SLOPES = {"P": (1.0, 0.5), "I": (0.1, 0.25, 1.0), "Ib": (0.1,), "T": (1.0,), "Tp": (1.0,), "D": (0.1,)}
_SEEN = {}      # (instance, family) -> cases so far: the family's slopes in turn on every instance


def _case(group, B, H, W, dtype, fam, split=1, tpw=0, align=0, publish=False):
    want = plan(B, H, W, dtype, align, split, tpw)
    inst = INSTANCES[want["instance"]]
    slope = _SLOPES[fam][_SEEN.setdefault((inst, fam), 0) % len(_SLOPES[fam])]
    _SEEN[(inst, fam)] += 1
    name = "%s_%s_%s_%s_%dx%dx%d_t%d%s%s" % (group, inst, dtype, fam, B, H, W, tpw, "_a%d" % align if align else "", "" if split else "_nosplit")
    assert name not in CASES, name
    CASES[name] = dict(name=name, group=group, B=B, H=H, W=W, dtype=dtype, fam=fam, split=split, tpw=tpw, align=align, publish=publish, slope=slope,
                       want=want, inst=inst, seed=len(CASES) + 1)


WALK_NTX, WALK_TPW = (1, 2, 3, 4, 5, 7), (1, 2, 3, 4, 7)
# W: the walk.  H = 16 (one tile row), B = 2 (a walk ends at a frame boundary), every forced tpw on every row length, on all four instances:
#   full   uint8, W = 16 ntx        f32   float32 frames, the same shapes        mfma   float32 frames, no tables
#   u8     uint8, H = 14 and W = 16 ntx - 4: the same number of tiles, the last one partial both ways
for _ntx in WALK_NTX:
    for _t in WALK_TPW:
        _pub = _ntx == 7
        _case("W", 2, 16, 16 * _ntx, "u8", "I", tpw=_t, publish=_pub)
        _case("W", 2, 14, 16 * _ntx - 4, "u8", "I", tpw=_t, publish=_pub)
        _case("W", 2, 16, 16 * _ntx, "f32", "P", tpw=_t, publish=_pub)
        _case("W", 2, 16, 16 * _ntx, "f32", "I", split=0, tpw=_t, publish=_pub)
        if _ntx in (5, 7):
            _case("W", 2, 16, 16 * _ntx, "u8", "P", tpw=_t)
            _case("W", 2, 14, 16 * _ntx - 4, "u8", "P", tpw=_t)
            _case("W", 2, 16, 16 * _ntx, "f32", "I", tpw=_t)
            _case("W", 2, 16, 16 * _ntx, "f32", "P", split=0, tpw=_t)
for _ntx, _t in ((5, 2), (7, 3)):      # T and D on a walk with pairs, a tail and a shorter last workgroup
    for _fam in ("T", "D"):
        _case("W", 2, 16, 16 * _ntx, "u8", _fam, tpw=_t)
        _case("W", 2, 14, 16 * _ntx - 4, "u8", _fam, tpw=_t)
        _case("W", 2, 16, 16 * _ntx, "f32", _fam, tpw=_t)
        _case("W", 2, 16, 16 * _ntx, "f32", _fam, split=0, tpw=_t)
    _case("W", 2, 16, 16 * _ntx, "u8", "Tp", split=0, tpw=_t)
    _case("W", 2, 16, 16 * _ntx, "f32", "Tp", split=0, tpw=_t)
    _case("W", 2, 16, 16 * _ntx, "u8", "D", split=0, tpw=_t)
# the bench-size walk: 26 tiles in one workgroup and in two
for _t in (26, 13):
    _case("Wb", 2, 16, 416, "u8", "I", tpw=_t)
    _case("Wb", 2, 14, 412, "u8", "I", tpw=_t)
    _case("Wb", 2, 16, 416, "f32", "P", tpw=_t)
    _case("Wb", 2, 16, 416, "f32", "I", split=0, tpw=_t)

# R: two and three tile rows -- the patch rows shared between tile rows, top and bottom padding
for _H in (32, 48):
    _case("R", 2, _H, 16, "u8", "I")
    _case("R", 2, _H, 16, "u8", "P")
    _case("R", 2, _H, 12, "u8", "I")
    _case("R", 2, _H, 16, "f32", "P")
    _case("R", 2, _H, 16, "f32", "I")
    _case("R", 2, _H, 16, "f32", "I", split=0)
    _case("R", 2, _H, 16, "u8", "Tp", split=0)

# E: partial tiles both ways.  W % 4 == 0: the uint8 split instance with guarded stores, and the float32 one
for _H in (2, 6, 14, 18, 34):
    for _W in (4, 12, 20, 36, 52):
        _case("E", 2, _H, _W, "u8", "I", publish=_H == 14)
        _case("E", 2, _H, _W, "f32", "P", publish=_H == 14)
for _H, _W in ((14, 20), (34, 52)):
    for _dt in ("u8", "f32"):
        _case("E", 2, _H, _W, _dt, "T")
        _case("E", 2, _H, _W, _dt, "D")
# E2: W % 4 == 2 -- uint8 frames fall back to the fp32 MFMA kernel, float32 frames take the split instance
for _H in (6, 18):
    for _W in (2, 6, 18, 22, 34):
        _case("E2", 2, _H, _W, "u8", "Tp")
        _case("E2", 2, _H, _W, "u8", "D")
        _case("E2", 2, _H, _W, "f32", "P")
        _case("E2", 2, _H, _W, "f32", "I")

# A: uint8 frames at a byte offset into their buffer -> the fp32 MFMA kernel, nothing published; offset 0: the whole-tile split instance
for _a in (1, 2, 3):
    _case("A", 2, 32, 32, "u8", "Tp", align=_a, publish=True)
    _case("A", 2, 32, 32, "u8", "D", align=_a)
_case("A", 2, 32, 32, "u8", "I", publish=True)

# M: the published maximum where a window of padding alone would win it (Ib): partial tiles of the two guarded split instances, and a whole-tile one
for _H, _W in ((14, 20), (18, 36)):
    _case("M", 2, _H, _W, "u8", "Ib", publish=True)
    _case("M", 2, _H, _W, "f32", "Ib", publish=True)
_case("M", 2, 16, 48, "u8", "Ib", tpw=2, publish=True)

# L: the launcher's own rule.  The smallest shape at which production walks (tpw = 2), and the three shapes of the detector-level conv_1 test
RULE_SHAPE = (1024, 16, 64)
_case("L", 1024, 16, 64, "u8", "I", publish=True)
PRODUCTION_SHAPES = ((3, 64, 96), (2, 416, 416), (1, 32, 32))
for _B, _H, _W in PRODUCTION_SHAPES:
    _case("L", _B, _H, _W, "u8", "I")


def by_group(*groups):
    return [k for k in CASES.values() if k["group"] in groups]


def case_ids(*groups):
    return [k["name"] for k in by_group(*groups)]
