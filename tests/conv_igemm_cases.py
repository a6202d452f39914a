"""Helpers of tests/test_gpu_conv_igemm_edges.py and tests/test_conv_igemm_cases_cpu.py (no GPU): the tile schedule of the fp32 implicit-GEMM
kernel (csrc/conv_igemm.hip) restated in numpy, float64 / integer references of everything its epilogues do, operand families with an exact
expected result, and the case table.

Operand families (layer mode: x [B,H,W,Cin], w HWIO [ks,ks,Cin,N], bias [N]; batched mode: x [P,Mt,K], w [P,N,K]):

  A   integers in [-8, 8] everywhere (xproj and cstate of the gate cases too).  A product is at most 64 and K at most 9 x 128 in this table,
      so every partial sum, in any K order, under any split and tile schedule, is an integer below 2^24: expected = the integer result, bit
      for bit.  `As` is the same family drawn small and sparse (x in [-2, 2] at density 1/4, w in [-1, 1]) for the sigmoid and gate cases,
      whose activations saturate on large pre-activations.
  H   one-hot weights: output channel n copies input channel (7 n) % Cin at tap n % taps.  A transposed tile or a wrong K order moves whole
      channels / taps instead of changing a sum.
  D   full-mantissa values over 13 binades, no denormals; judged by the dot-product bound d_bar(), not bit for bit.

The model knows no MFMA: it computes each tile's block as the kernel's schedule assigns it (tile_of, the persistent walk, the split ranges,
the K order of the packed weights against the order the activation chunks are fetched in) and is compared with a direct convolution that
shares none of that."""
import numpy as np

SENTINEL32 = 0x7FC5A5A5      # a quiet NaN no kernel produces
KCH = 32

CFG_TILES = {"128x128": (128, 128, 256), "128x64": (128, 64, 256), "64x128": (64, 128, 256), "256x128": (256, 128, 512), "256x256": (256, 256, 1024)}
CFG_CODE = {"128x128": 0, "128x64": 1, "256x128": 2, "256x256": 3, "64x128": 4}
CFGS = ("128x128", "128x64", "64x128", "256x128", "256x256")
QUAD_KINDS = ("pool", "pool_both", "s2d")


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- the tile schedule
def tile_of(L, total, ntm, ntn, tile_gn, gw_is_gn=False):
    """conv_igemm_f32's tile_of: linear index L -> (z, tile_m, tile_n).  gw_is_gn: the defect `gw` replaced by `gn`."""
    q, r = total >> 3, total & 7
    xcd, j = L & 7, L >> 3
    t = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + j
    ntiles = ntm * ntn
    z, bid = divmod(t, ntiles)
    gn = tile_gn if 0 < tile_gn < ntn else ntn
    per_group = gn * ntm
    grp, rem = divmod(bid, per_group)
    gw = gn if gw_is_gn else min(gn, ntn - grp * gn)
    tile_m = rem // gw
    return z, tile_m, grp * gn + (rem - tile_m * gw)


def tile_gn_of(ks, kind):
    """launch_conv_igemm: column tiles per group"""
    return 1 if ks == 3 and kind != "gates" else 2


def split_ranges(nk_all, S):
    """chunk ranges [k0, k0 + nk) of the S splits (blockIdx.y = y of gridDim.y = S)"""
    return [(nk_all * y // S, nk_all * (y + 1) // S - nk_all * y // S) for y in range(S)]


def k_index(ci, tap, taps):
    """position of (input channel, tap) in the packed K axis: channel-slice outer, tap inner"""
    return ((ci // KCH) * taps + tap) * KCH + ci % KCH


class Schedule:
    """Which workgroup computes which tile on which turn: G workgroups, workgroup b takes L = b, b + G, ... < total."""

    def __init__(self, M, N, BM, BN, P, tile_gn, G, gw_is_gn=False):
        self.M, self.N, self.BM, self.BN, self.P, self.tile_gn, self.G = M, N, BM, BN, max(P, 1), tile_gn, G
        self.ntm, self.ntn = _cdiv(M, BM), _cdiv(N, BN)
        self.total = self.ntm * self.ntn * self.P
        self.gw_is_gn = gw_is_gn
        self.tiles = [tile_of(L, self.total, self.ntm, self.ntn, tile_gn, gw_is_gn) for L in range(self.total)]

    def walk(self):
        """yields (workgroup, turn, L, (z, tile_m, tile_n))"""
        for b in range(min(self.G, self.total)):
            for turn, L in enumerate(range(b, self.total, self.G)):
                yield b, turn, L, self.tiles[L]

    def is_bijection(self):
        want = {(z, tm, tn) for z in range(self.P) for tm in range(self.ntm) for tn in range(self.ntn)}
        return len(set(self.tiles)) == self.total and set(self.tiles) == want

    def max_turns(self):
        return _cdiv(self.total, min(self.G, self.total))

    def locate(self, z, m, n, nk_all=None, ksplit=1):
        """where output (z, row m, column n) is computed: tile, workgroup, turn and -- for split-K -- the chunk ranges"""
        key = (z, m // self.BM, n // self.BN)
        L = self.tiles.index(key)
        d = {"L": L, "z": z, "m0": key[1] * self.BM, "n0": key[2] * self.BN, "workgroup": L % self.G, "turn": L // self.G}
        if ksplit > 1:
            d["splits"] = split_ranges(nk_all, ksplit)
        return d


def bijective(total, G, ntn, gn):
    """every tile of a total-tile launch (ntn column tiles, total % ntn == 0, one problem) is visited exactly once by G workgroups"""
    ntm = total // ntn
    seen = []
    for b in range(min(G, total)):
        for L in range(b, total, G):
            seen.append(tile_of(L, total, ntm, ntn, gn))
    return len(seen) == total and set(seen) == {(0, tm, tn) for tm in range(ntm) for tn in range(ntn)}


# ---------------------------------------------------------------------------------------------------------------- row orders
def quad_rows(B, H, W):
    """ORD_QUAD: m = ((b H/2 + h2) W/2 + w2) 4 + dy 2 + dx -> arrays (b, h, w) of length B H W"""
    m = np.arange(B * H * W)
    q, d = m >> 2, m & 3
    W2, hw2 = W // 2, (H // 2) * (W // 2)
    b, r = q // hw2, q % hw2
    return b, 2 * (r // W2) + (d >> 1), 2 * (r % W2) + (d & 1)


def linear_rows(B, H, W):
    m = np.arange(B * H * W)
    return m // (H * W), (m % (H * W)) // W, m % W


# ---------------------------------------------------------------------------------------------------------------- references
def _acc_dtype(*arrays):
    return np.int64 if all(np.all(a == np.rint(a)) for a in arrays) else np.float64


def conv_same(x, w):
    """Conv2D 'same' stride 1, NHWC x HWIO -> [B,H,W,N]; int64 on integer operands (exact), float64 otherwise"""
    dt = _acc_dtype(x, w)
    x, w = np.asarray(x).astype(dt), np.asarray(w).astype(dt)
    B, H, W, _ = x.shape
    ks = w.shape[0]
    p = ks // 2
    xp = np.zeros((B, H + 2 * p, W + 2 * p, x.shape[3]), dt)
    xp[:, p:p + H, p:p + W] = x
    out = np.zeros((B, H, W, w.shape[3]), dt)
    for dy in range(ks):
        for dx in range(ks):
            out += xp[:, dy:dy + H, dx:dx + W] @ w[dy, dx]
    return out


def conv_abs(x, w, bias):
    """sum_k |a||w| + |b|: the scale of family D's bound"""
    s = conv_same(np.abs(np.asarray(x, np.float64)) + 0.0, np.abs(np.asarray(w, np.float64)) + 0.0).astype(np.float64)
    return s + (np.abs(np.asarray(bias, np.float64)) if bias is not None else 0.0)


def act32(z, bias, slope):
    """the epilogue on an exact pre-activation: float32(z + b), LeakyReLU as ONE float32 multiply"""
    v = (np.asarray(z, np.float64) + (np.asarray(bias, np.float64) if bias is not None else 0.0)).astype(np.float32)
    return np.where(v > 0, v, v * np.float32(slope)).astype(np.float32)


def sigmoid64(z, bias):
    v = np.asarray(z, np.float64) + (np.asarray(bias, np.float64) if bias is not None else 0.0)
    return 1.0 / (1.0 + np.exp(-v))


def maxpool2(v):
    B, H, W, C = v.shape
    return v.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def space_to_depth2(v):
    """tf.space_to_depth(2): channel (dy 2 + dx) C + c"""
    B, H, W, C = v.shape
    return v.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C)


def gate_columns(U):
    """packed column n' = (j/32) 128 + g 32 + j%32 <- Keras column g U + j; returns n_map [4U]"""
    n = np.arange(4 * U)
    return ((n % 128) // 32) * U + (n // 128) * 32 + n % 32


def hard_sigmoid32(z):
    """clip(fma(0.2f, z, 0.5f), 0, 1): float32 coefficient, exact product and sum in float64 (z an integer), rounded ONCE"""
    y = (np.float64(np.float32(0.2)) * np.asarray(z, np.float64) + 0.5).astype(np.float32)
    return np.clip(y, np.float32(0), np.float32(1))


def gate_update(z_keras, c):
    """z_keras [..., 4U] exact pre-activations in Keras order (i, f, c, o), c [..., U] -> (c_new, h) in float64"""
    U = c.shape[-1]
    zi, zf, zc, zo = (np.asarray(z_keras[..., g * U:(g + 1) * U], np.float64) for g in range(4))
    c_new = hard_sigmoid32(zf).astype(np.float64) * np.asarray(c, np.float64) + hard_sigmoid32(zi).astype(np.float64) * np.tanh(zc)
    return c_new, hard_sigmoid32(zo).astype(np.float64) * np.tanh(c_new)


def d_bar(K, ksplit):
    """family D: bar on |got - ref| / (sum |a||w| + |b|) -- the bound of a length-K float32 dot product in any order (K roundings), the adds
    of the split partials, the bias add and the activation multiply, times 2 for the MFMA's undocumented internal rounding"""
    return 2.0 * (K + max(ksplit, 1) + 2) * 2.0 ** -24


SIGMOID_BAR = 2.0 ** -21      # absolute: a 1-ulp expf, the add and the divide on outputs <= 1, times 2
GATE_RTOL, GATE_ATOL = 1e-4, 2e-5      # the project's bar for the ConvLSTM step (test_convlstm_step_vs_oracle)


# ---------------------------------------------------------------------------------------------------------------- operands
def operands(k):
    """the case's operands as float32 numpy arrays: dict(x, w, bias[, xproj, cstate]); batched cases: x [P,Mt,K], w [P,N,K]"""
    rs = np.random.RandomState(k["seed"])
    fam, ks, Cin, N = k["fam"], k["ks"], k["Cin"], k["N"]
    P = k["P"]
    if P > 1:
        xs, ws = (P, k["W"], Cin), (P, N, Cin)
    else:
        xs, ws = (k["B"], k["H"], k["W"], Cin), (ks, ks, Cin, N)
    o = {}
    if fam == "A":
        o["x"], o["w"] = rs.randint(-8, 9, xs), rs.randint(-8, 9, ws)
    elif fam == "As":
        o["x"], o["w"] = rs.randint(-2, 3, xs) * (rs.randint(0, 4, xs) == 0), rs.randint(-1, 2, ws)
    elif fam == "H":
        assert P <= 1
        o["x"] = rs.randint(-8, 9, xs)
        w = np.zeros(ws)
        n = np.arange(N)
        tap = n % (ks * ks)
        w[tap // ks, tap % ks, (7 * n) % Cin, n] = 1.0
        o["w"] = w
    elif fam == "D":
        o["x"] = rs.randn(*xs) * np.exp2(rs.randint(-6, 7, xs))
        o["w"] = rs.randn(*ws) * np.exp2(rs.randint(-3, 4, ws)) / np.sqrt(ks * ks * Cin)
    else:
        raise KeyError(fam)
    o["bias"] = None
    if k["bias"]:
        o["bias"] = rs.randn(N) if fam == "D" else rs.randint(-8, 9, N)
    if k["kind"] == "gates":
        M, U = k["B"] * k["H"] * k["W"], N // 4
        o["xproj"], o["cstate"] = rs.randint(-8, 9, (M, N)), rs.randint(-8, 9, (M, U))      # xproj in PACKED column order
    return {n: (None if a is None else np.ascontiguousarray(a, dtype=np.float32)) for n, a in o.items()}


def preact(k, o):
    """exact pre-activation Z [P][M][N] WITHOUT bias, rows in the kind's row order (linear, or quad for the pooling kinds), columns in Keras order"""
    if k["P"] > 1:
        dt = _acc_dtype(o["x"], o["w"])
        return np.einsum("pmk,pnk->pmn", o["x"].astype(dt), o["w"].astype(dt))
    y = conv_same(o["x"], o["w"])
    B, H, W = k["B"], k["H"], k["W"]
    b, h, w = quad_rows(B, H, W) if k["kind"] in QUAD_KINDS else linear_rows(B, H, W)
    return y[b, h, w][None]


def pack_weights(w, n_map=None):
    """pack_conv_weights restated: HWIO [ks,ks,Cin,N] -> [N][K], k = ((ci/32) taps + tap) 32 + ci%32"""
    ks, _, Cin, N = w.shape
    taps = ks * ks
    ci = np.arange(Cin)
    out = np.zeros((N, taps * Cin), w.dtype)
    for t in range(taps):
        out[:, k_index(ci, t, taps)] = w[t // ks, t % ks].T
    return out if n_map is None else out[n_map]


def model_preact(k, o, BM, BN, G, mutate=None):
    """Z [P][M][N] computed AS SCHEDULED: the A rows gathered chunk by chunk in the order the kernel fetches them, against the packed weights,
    tile by tile along the persistent walk, split by split.  Rows / columns nobody computed stay NaN.  mutate:
      "tap_outer"   the activation chunks fetched tap-outer / channel-slice-inner while the weights keep their packed order
      "split_shift" every split but the first starts one chunk late
      "gw_is_gn"    tile_of without the narrower last column group
      "stale_rows"  a workgroup keeps its first tile's row pointers (problem and row tile) on its later turns"""
    ks, Cin, N, P = k["ks"], k["Cin"], k["N"], max(k["P"], 1)
    taps = ks * ks
    K = taps * Cin
    dt = _acc_dtype(o["x"], o["w"])
    if k["P"] > 1:
        A, Wt = o["x"].astype(dt), o["w"].astype(dt)
        M = k["W"]
    else:
        B, H, W = k["B"], k["H"], k["W"]
        M = B * H * W
        b, h, w = quad_rows(B, H, W) if k["kind"] in QUAD_KINDS else linear_rows(B, H, W)
        x = o["x"].astype(dt)
        A = np.zeros((1, M, K), dt)
        cpt = Cin // KCH
        for kc in range(taps * cpt):
            cc, tap = (kc % cpt, kc // cpt) if mutate == "tap_outer" else (kc // taps, kc % taps)
            ih, iw = h + (tap // ks - ks // 2), w + (tap % ks - ks // 2)
            ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            A[0, ok, kc * KCH:(kc + 1) * KCH] = x[b[ok], ih[ok], iw[ok], cc * KCH:(cc + 1) * KCH]
        Wt = pack_weights(o["w"].astype(dt))[None]
    S = max(k["ksplit"], 1)
    ranges = split_ranges(K // KCH, S)
    if mutate == "split_shift":
        ranges = [(k0 + (y > 0), nk - (y > 0)) for y, (k0, nk) in enumerate(ranges)]
    sch = Schedule(M, N, BM, BN, P, tile_gn_of(ks, k["kind"]), G, gw_is_gn=(mutate == "gw_is_gn"))
    Z = np.full((P, M, N), np.nan)
    first = {}
    for wg, turn, L, (z, tm, tn) in sch.walk():
        first.setdefault(wg, (z, tm))
        az, atm = first[wg] if mutate == "stale_rows" else (z, tm)
        if z >= P or tn >= sch.ntn or tm >= sch.ntm:
            continue      # (a defective tile map may point outside; the kernel would write out of bounds -- the model just drops it)
        rows = slice(tm * BM, min((tm + 1) * BM, M))
        arows = slice(atm * BM, atm * BM + (rows.stop - rows.start))
        cols = slice(tn * BN, min((tn + 1) * BN, N))
        acc = 0
        for k0, nk in ranges:
            ksl = slice(k0 * KCH, (k0 + nk) * KCH)
            a = A[az, arows, ksl]
            if a.shape[0] < rows.stop - rows.start:
                a = np.concatenate([a, np.zeros((rows.stop - rows.start - a.shape[0], a.shape[1]), dt)])
            acc = acc + a @ Wt[z, cols, ksl].T
        Z[z, rows, cols] = acc
    return Z


# ---------------------------------------------------------------------------------------------------------------- what must run
def expected_info(k, cus=256):
    """what dt_conv_igemm must report for the case: the instance (resolved cfg, BM, BN, threads, persistent) and the grid"""
    cfg = k.get("runs", k["cfg"])      # "runs": the configuration after the 256x256 fallback / the gate and split-K instances' own
    split = k["ksplit"] > 1
    if k["kind"] == "gates":
        BM, BN, threads = (256, 256, 1024) if cfg == "256x256" else (128, 128, 256)
    else:
        BM, BN, threads = CFG_TILES[cfg]
    P = max(k["P"], 1)
    M = k["W"] if k["P"] > 1 else k["B"] * k["H"] * k["W"]
    total = _cdiv(M, BM) * _cdiv(k["N"], BN) * P
    persistent = int(k["ks"] == 1 and k["kind"] == "plain" and not split)
    grid = total
    if persistent:
        slots = cus * (1 if threads > 256 else 2) // 8 * 8
        grid = min(grid, slots)
        if k["wg_cap"]:
            grid = min(grid, k["wg_cap"])
    return {"cfg": CFG_CODE[cfg], "BM": BM, "BN": BN, "threads": threads, "persistent": persistent, "grid_x": grid, "grid_y": max(k["ksplit"], 1) if split else 1,
            "total": total}


def instance_of(k):
    """the template instance a case runs, as a readable key"""
    e = expected_info(k)
    cfg = k.get("runs", k["cfg"])
    if k["kind"] == "gates":
        return "gates %dx%d %s" % (k["ks"], k["ks"], cfg)
    if k["ksplit"] > 1:
        return "partial %dx%d" % (k["ks"], k["ks"])
    return "%s %dx%d %s%s" % (k["kind"], k["ks"], k["ks"], cfg, " persistent" if e["persistent"] else "")


ALL_INSTANCES = sorted(["%s %dx%d %s%s" % (kind, ks, ks, cfg, " persistent" if (kind == "plain" and ks == 1) else "")
                        for kind, ks in (("plain", 3), ("plain", 1), ("pool", 3), ("pool", 1), ("pool_both", 3), ("s2d", 1)) for cfg in CFGS] +
                       ["gates 3x3 128x128", "gates 3x3 256x256", "gates 1x1 128x128", "partial 3x3", "partial 1x1"])
assert len(ALL_INSTANCES) == 35


# ---------------------------------------------------------------------------------------------------------------- the case table
CASES = {}


def _case(name, group, ks, B, H, W, Cin, N, kind="plain", cfg="128x128", fam="A", P=0, bias=True, slope=1.0, act=0, ksplit=0, npad=0, wg_cap=0,
          publish=False, in_ld=0, in_gap=0, out_extra=0, out2_extra=0, col_off=0, xp_extra=0, c_extra=0, runs=None, pins=()):
    """in_ld: pixel stride (0 = Cin); in_gap: floats between frames; out_extra / out2_extra / xp_extra / c_extra: row stride beyond the columns
    written; col_off: the output starts at this column of its rows (as conv_20 writes into the concat buffer); pins: the structural claims the
    case makes ("korder", "split", "gw", "turns"), each proven sensitive on the model by the CPU suite"""
    assert name not in CASES, name
    k = dict(name=name, group=group, ks=ks, B=B, H=H, W=W, Cin=Cin, N=N, kind=kind, cfg=cfg, fam=fam, P=P, bias=bias and P <= 1 and kind != "gates",
             slope=slope, act=act, ksplit=ksplit, npad=npad, wg_cap=wg_cap, publish=publish, in_ld=in_ld or Cin, in_gap=in_gap, out_extra=out_extra,
             out2_extra=out2_extra, col_off=col_off, xp_extra=xp_extra, c_extra=c_extra, pins=tuple(pins), seed=len(CASES) + 1)
    if runs:
        k["runs"] = runs
    CASES[name] = k


def _frames(M):
    """(B, H, W) of M rows for a plain layer: one frame of 1 x M"""
    return 1, 1, M


for _cfg in CFGS:
    _BM = CFG_TILES[_cfg][0]
    for _ks in (3, 1):
        for _M in (_BM - 1, _BM, _BM + 1):      # R: the row edge of every plain instance (the 1x1 ones are the persistent kernels, one tile each)
            _case("R_%dx%d_%s_M%d" % (_ks, _ks, _cfg, _M), "R", _ks, 1, 1, _M, 32, 128, cfg=_cfg, slope=0.1)
        for _N in (1, 63, 64, 65, 85, 127, 129, 255, 257, 384):      # C: the column edge; M = 130 = 2 x 5 x 13: two or three row tiles but for 256-row ones
            _case("C_%dx%d_%s_N%d" % (_ks, _ks, _cfg, _N), "C", _ks, 2, 5, 13, 32, _N, cfg=_cfg, slope=0.1, out_extra=4 - _N % 4,
                  pins=("gw",) if (_ks == 1 and _N == 384 and _cfg in ("128x128", "64x128")) else ())      # (more than one row tile)
# R: a tile that spans frames (5 frames of 5 x 5 = 125 rows + 1 more frame: B = 6 gives 150 rows, two 128-row tiles), and the 'same' masks of thin frames
_case("R_3x3_frames_5x5", "R", 3, 6, 5, 5, 32, 128, slope=0.1)
_case("R_3x3_frames_5x5_64", "R", 3, 5, 5, 5, 32, 128, cfg="64x128", slope=0.1)
_case("R_3x3_W1", "R", 3, 2, 67, 1, 32, 128, slope=0.1)
_case("R_3x3_H1W1", "R", 3, 131, 1, 1, 32, 128, slope=0.1)
# C: with the weight rows a loaded layer has (N rounded up to 256) 257 columns run the 256x256 tile itself; with 384 rows it must fall back
for _ks in (3, 1):
    _case("C_%dx%d_256x256_N257_npad384" % (_ks, _ks), "C", _ks, 2, 5, 13, 32, 257, cfg="256x256", npad=384, runs="256x128", slope=0.1, out_extra=3)

for _ks in (3, 1):      # K: the chunk order across taps and channel slices
    for _Cin in (32, 64, 96):
        for _fam in ("A", "H", "D"):
            _case("K_%dx%d_Cin%d_%s" % (_ks, _ks, _Cin, _fam), "K", _ks, 2, 7, 10, _Cin, 128, fam=_fam, slope=1.0 if _fam == "D" else 0.1,
                  pins=("korder",) if (_ks == 3 and _Cin > 32 and _fam != "D") else ())

# S: strides -- pixel stride 80 for 64 channels, three rows of padding between frames, rows 12 floats longer than N, the output at a column offset
_case("S_3x3_strided", "S", 3, 3, 6, 7, 64, 72, in_ld=80, in_gap=3 * 7 * 80, out_extra=12, slope=0.1)
_case("S_3x3_col_offset", "S", 3, 3, 6, 7, 64, 72, in_ld=80, in_gap=3 * 7 * 80, out_extra=12 + 256, col_off=256, slope=0.1)
_case("S_1x1_strided_out", "S", 1, 3, 6, 7, 64, 72, in_ld=80, out_extra=12 + 256, col_off=256, slope=0.1)      # (1x1 linear: dense frames; the pixel stride may exceed Cin)

# P: the persistent walk.  7 row tiles on 3 workgroups: turns 3 / 2 / 2
_case("P1_K32", "P", 1, *_frames(7 * 128 - 5), 32, 128, bias=False, wg_cap=3, pins=("turns",))
_case("P2_K96_bias_leaky", "P", 1, *_frames(7 * 128 - 5), 96, 128, slope=0.1, wg_cap=3, pins=("turns",))
# batched: P = 3 of 2 x 2 tiles: total 12 (q = 1, r = 4) on 5 workgroups; P = 36 as F(4x4) has, on 40; fewer than 8 tiles (q = 0)
_case("P3_P3_2x2_cap5", "P", 1, 1, 1, 130, 64, 256, P=3, wg_cap=5, out_extra=4, pins=("turns",))
_case("P3_P36_cap40", "P", 1, 1, 1, 130, 32, 256, P=36, wg_cap=40, pins=("turns",))
_case("P3_total6", "P", 1, 1, 1, 130, 32, 129, P=3, wg_cap=4, out_extra=3, pins=("turns",))
_case("P3_P3_3cols_cap5", "P", 1, 1, 1, 130, 32, 384, P=3, wg_cap=5, pins=("turns", "gw"))
for _cfg in ("64x128", "128x64", "256x128", "256x256"):      # P4: the other persistent instances, two workgroups
    _BM, _BN, _ = CFG_TILES[_cfg]
    _case("P4_%s" % _cfg, "P", 1, 1, 1, 2 * _BM + 3, 64, 2 * _BN, P=2, cfg=_cfg, wg_cap=2, pins=("turns",))
# P6: the raw form (no bias, linear) publishing its maximum
_case("P6_raw_publish", "P6", 1, *_frames(5 * 128 - 7), 64, 130, bias=False, publish=True, wg_cap=2, out_extra=2)
_case("P6_raw_publish_batchless_256", "P6", 1, *_frames(3 * 256 - 7), 64, 256, cfg="256x256", bias=False, publish=True, wg_cap=2)
# the general persistent epilogue publishing (bias): the path production takes for 1x1 layers
_case("P6_bias_publish", "P6", 1, *_frames(5 * 128 - 7), 64, 130, slope=0.1, publish=True, wg_cap=2, out_extra=2)

# Dh: the heat-map tracker's Dense(sigmoid) head
_case("Dh_sigmoid_head", "Dh", 1, 70, 1, 1, 64, 1056, fam="As", act=1)

# Q: the quad row order and its epilogues.  M = 4, 120, 132 (crosses a 128-row tile), 780
for _i, (_B, _H, _W) in enumerate(((1, 2, 2), (2, 6, 10), (1, 6, 22), (3, 10, 26))):
    for _cfg in CFGS:
        _pub = _i == 2 and _cfg == "128x128"
        _case("Q_pool_3x3_%s_%dx%dx%d" % (_cfg, _B, _H, _W), "Q", 3, _B, _H, _W, 32, 72, kind="pool", cfg=_cfg, slope=0.1, out_extra=8, publish=_pub)
        _case("Q_pool_1x1_%s_%dx%dx%d" % (_cfg, _B, _H, _W), "Q", 1, _B, _H, _W, 32, 72, kind="pool", cfg=_cfg, slope=0.1, out_extra=8, publish=_pub)
        _case("Q_both_3x3_%s_%dx%dx%d" % (_cfg, _B, _H, _W), "Q", 3, _B, _H, _W, 32, 72, kind="pool_both", cfg=_cfg, slope=0.1, out_extra=8, out2_extra=20,
              publish=_pub)
        _case("Q_s2d_1x1_%s_%dx%dx%d" % (_cfg, _B, _H, _W), "Q", 1, _B, _H, _W, 32, 72, kind="s2d", cfg=_cfg, slope=0.1, out_extra=8, publish=_pub)

# SK: split-K.  nk_all chunks over S splits: mid-tap starts (9 over 2, 4; 18 over 5), one chunk per split (9 over 9), a split that crosses the
# 32-channel slice (18 over 5: [3,7) [7,10) [10,14)); 36 over 6; the 1x1 forms
for _ks, _Cin, _S in ((3, 32, 2), (3, 32, 4), (3, 32, 9), (3, 64, 5), (3, 128, 6), (1, 96, 2), (1, 384, 2)):
    _case("SK_%dx%d_Cin%d_S%d" % (_ks, _ks, _Cin, _S), "SK", _ks, 1, 3, 43, _Cin, 85, ksplit=_S, slope=0.1, out_extra=7, pins=("split",))
for _ks, _Cin, _S in ((3, 64, 5), (1, 96, 2)):      # ... and on full-mantissa operands, at the bound with ksplit in it
    _case("SK_%dx%d_Cin%d_S%d_D" % (_ks, _ks, _Cin, _S), "SK", _ks, 1, 3, 43, _Cin, 85, ksplit=_S, fam="D", out_extra=7)

# G: the gate epilogue.  N = 4 U in Keras order on the host, packed [j/32][gate][j%32] on the device
for _U in (32, 64, 96, 128):
    for _M in (63, 130):
        _B, _H, _W = (1, 7, 9) if _M == 63 else (2, 5, 13)
        _case("G_3x3_U%d_M%d" % (_U, _M), "G", 3, _B, _H, _W, 32, 4 * _U, kind="gates", fam="As", xp_extra=8, c_extra=4, out_extra=12)
        _case("G_1x1_U%d_M%d" % (_U, _M), "G", 1, _B, _H, _W, 32, 4 * _U, kind="gates", fam="As", xp_extra=8, c_extra=4, out_extra=12)
        # 16 waves where 4 U is a multiple of 256; U = 32 / 96 must report the fallback to the 128x128 gate instance
        _case("G_3x3_256_U%d_M%d" % (_U, _M), "G", 3, _B, _H, _W, 32, 4 * _U, kind="gates", cfg="256x256", fam="As", xp_extra=8, c_extra=4, out_extra=12,
              runs="256x256" if _U % 64 == 0 else "128x128")


def by_group(group):
    return [k for k in CASES.values() if k["group"] == group]


def case_ids(group):
    return [k["name"] for k in by_group(group)]
