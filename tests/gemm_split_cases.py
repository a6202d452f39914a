"""Helpers of tests/test_gpu_gemm_split_edges.py and tests/test_gemm_split_cases_cpu.py (no GPU): operand families for which the split
GEMM (csrc/wino_gemm_s3.hip) has an expected result that is exact, the kernel's tile map restated, a numpy model of its arithmetic
with one partial product removable, and the case table.

Operand families, each a function of (P, Mt, K, N, seed) -> float32 v [P, Mt, K], u [P, N, K]:

  A  small integers in [-8, 8].  Both splits carry them in their first term alone (the fp16 form scales by powers of two), every partial
     sum is an integer below 2^24: expected = the integer product, bit for bit, in both forms.  Sees the leading product only.
  B  n (1 + 2^-13), n in 1..8; v with at most 8 non-zeros per row, u dense, all positive.  hi = n and lo = n 2^-13 in BOTH splits, the
     sums of hi hi and of the cross products fit in 24 bits in any order, what is left out (lo lo, 2^-26 of the result) lies below a
     quarter of the result's last place: expected = float32(float64 product), bit for bit.  Sees the cross products.
  D  13 binades, heavy tails (the generator of test_split_bf16_gemm_benched_shapes_against_float64).  Judged at that test's absolute
     bars: error relative to sum_k |v||u|, rms < 1.5 x 2^-24 and max < 32 x 2^-24.  Sees the three smallest products of the bf16 form,
     which are zero (or vanish in the rounding) on A and B."""
import numpy as np

from test_split_arith import h2_base, split2, split3

D_RMS_BAR = 1.5 * 2.0 ** -24
D_MAX_BAR = 32 * 2.0 ** -24
B_EPS = 2.0 ** -13


# ---------------------------------------------------------------------------------------------------------------- operand families
def family_a(P, Mt, K, N, seed):
    rs = np.random.RandomState(seed)
    v = rs.randint(-8, 9, (P, Mt, K)).astype(np.float32)
    u = rs.randint(-8, 9, (P, N, K)).astype(np.float32)
    return v, u


def family_b(P, Mt, K, N, seed):
    rs = np.random.RandomState(seed)
    f = np.float32(1.0 + B_EPS)                                    # n (1 + 2^-13) has at most 17 significant bits: exact in float32
    v = np.zeros((P, Mt, K), np.float32)
    where = rs.randint(0, K, (P, Mt, 8))                           # 8 draws with replacement: at most 8 non-zeros per row
    np.put_along_axis(v, where, rs.randint(1, 9, (P, Mt, 8)).astype(np.float32) * f, axis=2)
    u = rs.randint(1, 9, (P, N, K)).astype(np.float32) * f
    return v, u


def family_d(P, Mt, K, N, seed):
    rs = np.random.RandomState(seed)
    v = rs.randn(P, Mt, K).astype(np.float32) * np.exp2(rs.randint(-6, 7, (P, Mt, K))).astype(np.float32)
    u = rs.randn(P, N, K).astype(np.float32) * np.exp2(rs.randint(-3, 4, (P, N, K))).astype(np.float32) / np.float32(np.sqrt(K))
    return v, u.astype(np.float32)


FAMILIES = {"A": family_a, "B": family_b, "D": family_d}


def d_error(got, ref64, scale64):
    """family D's measure: (rms, max) of |got - ref| / sum_k |v||u| (numpy, float64 reference)"""
    e = np.abs(np.asarray(got, np.float64) - ref64) / scale64
    return float(np.sqrt(np.mean(e * e))), float(e.max())


def d_passes(rms, mx):
    return rms < D_RMS_BAR and mx < D_MAX_BAR


# ---------------------------------------------------------------------------------------------------------------- the tile map
def _cdiv(a, b):
    return -(-a // b)


class TileMap:
    """wino_gemm_s3.hip's persistent tile loop (s3_body: tile_of, `first`; launch_wino_gemm_s3: the grid; wino_gemm_s3_half_chosen).
    Tile L = (p MT + mt) NTL + nt; G workgroups; workgroup w starts at (w & 7)(G >> 3) + (w >> 3) if G % 8 == 0, else at w, and
    walks with stride G.  `half` as the entry points take it: 1 / -1 force the 128-row form on / off, 0 lets the launcher choose."""

    def __init__(self, P, Mt, N, half, cus):
        self.BN = 256 if N % 256 == 0 else 128
        self.half_form = False
        if self.BN == 256:
            t, th = P * _cdiv(Mt, 256) * (N // 256), P * _cdiv(Mt, 128) * (N // 256)
            rounds, rounds_h = _cdiv(t, cus), _cdiv(th, 2 * cus)
            self.half_form = half > 0 or (half == 0 and rounds <= 8 and rounds_h < rounds)
        self.BM = 128 if self.half_form else 256
        self.P, self.MT, self.NTL = P, _cdiv(Mt, self.BM), _cdiv(N, self.BN)
        self.tiles = P * self.MT * self.NTL
        self.G = min(self.tiles, (2 if self.half_form else 1) * cus)
        self.xcd_order = self.G % 8 == 0

    def first(self, w):
        return (w & 7) * (self.G >> 3) + (w >> 3) if self.xcd_order else w

    def sequence(self, w):
        return list(range(self.first(w), self.tiles, self.G))

    def max_turns(self):
        return _cdiv(self.tiles, self.G)

    def locate(self, p, m, n):
        """(tile, workgroup, turn) of output element (p, m, n)"""
        L = (p * self.MT + m // self.BM) * self.NTL + n // self.BN
        turn, f = divmod(L, self.G)
        w = (f % (self.G >> 3)) * 8 + f // (self.G >> 3) if self.xcd_order else f
        return L, w, turn

    def tag(self):
        return "s3_tile:128x2" if self.half_form else "s3_tile:256"


# ---------------------------------------------------------------------------------------------------------------- the numpy model
# partial products, smallest first, as (term of U, term of V): S3Prod<3> / S3Prod<2> of the kernel
PRODUCTS = {3: ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)), 2: ((1, 0), (0, 1), (0, 0))}
PRODUCT_NAMES = {3: ("u3v1", "u2v2", "u1v3", "u2v1", "u1v2", "u1v1"), 2: ("ulo_vhi", "uhi_vlo", "uhi_vhi")}


def model_gemm(v, u, nt, drop=None, bias=None, slope=1.0):
    """The kernel's arithmetic of test_split_arith.py at GEMM level: v [P, Mt, K] x u [P, N, K] -> float32 [P, Mt, N].  nt = 3: three bf16
    terms, six products; nt = 2: two fp16 terms of the scaled operands (V by one power of two from the whole tensor's max |v|, U per
    plane), three products.  Per 16 k and product: the exact block sum, rounded into the float32 accumulator once.  `drop`: index
    into PRODUCTS[nt] of a product to leave out.  `bias` [N] as the 1x1 layers carry it: one extra K stage of b x 1.0 in the bf16
    form, one fma in the fp16 form's epilogue; `slope`: LeakyReLU."""
    v, u = np.asarray(v, np.float32), np.asarray(u, np.float32)
    P, Mt, K = v.shape
    N = u.shape[1]
    assert K % 16 == 0
    if nt == 3:
        vt, ut = [t.astype(np.float64) for t in split3(v)], [t.astype(np.float64) for t in split3(u)]
        back = np.ones(P, np.float32)
    else:
        bv, iv = h2_base(np.abs(v).max())
        bu = [h2_base(np.abs(u[p]).max()) for p in range(P)]
        vt = [t.astype(np.float64) for t in split2(v * bv)]
        ut = [t.astype(np.float64) for t in split2(u * np.array([b for b, _ in bu], np.float32)[:, None, None])]
        back = np.array([i * iv for _, i in bu], np.float32)
    acc = np.zeros((P, Mt, N), np.float32)
    for k0 in range(0, K, 16):
        s = slice(k0, k0 + 16)
        for pi, (a, b) in enumerate(PRODUCTS[nt]):
            if pi == drop:
                continue
            acc = (acc.astype(np.float64) + np.einsum("pmk,pnk->pmn", vt[b][..., s], ut[a][..., s])).astype(np.float32)
    if nt == 3:
        if bias is not None:      # the bias stage: A = (1, 0, 0) as terms, so u3v1, u2v1, u1v1 carry the bias's three terms
            bt = split3(np.asarray(bias, np.float32))
            for pi, (a, b) in enumerate(PRODUCTS[3]):
                if b == 0 and pi != drop:
                    acc = (acc.astype(np.float64) + bt[a].astype(np.float64)).astype(np.float32)
    else:
        bl = np.zeros(N, np.float64) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
        acc = (acc.astype(np.float64) * back.astype(np.float64)[:, None, None] + bl).astype(np.float32)      # powers of two: one rounding
    return np.where(acc > 0, acc, acc * np.float32(slope)).astype(np.float32)


def reference(v, u):
    """float64 product and sum_k |v||u| (numpy)"""
    v64, u64 = np.asarray(v, np.float64), np.asarray(u, np.float64)
    return np.einsum("pmk,pnk->pmn", v64, u64), np.einsum("pmk,pnk->pmn", np.abs(v64), np.abs(u64))


# ---------------------------------------------------------------------------------------------------------------- the case table
# Sizes marked CU are functions of the device's CU count: enough tiles that some workgroup runs three (2.5 x the grid, rounded up).
def _turnover_mt(cus, P, ntl, bm, wg_per_cu):
    """row tiles MT with P * MT * ntl >= 2.5 * wg_per_cu * cus, and the Mt that leaves ONE live row in the last of them"""
    mt = _cdiv(5 * wg_per_cu * cus, 2 * P * ntl)
    return bm * mt - (bm - 1)


# Through ctx.gemm_split, the Winograd-operand instances: name -> (shape(cus) -> (P, Mt, K, N, half), turn-over premise)
WINO_CASES = {
    "one_row_k32": (lambda cus: (1, 1, 32, 128, -1), False),                    # one tile, one live row, 2 stages against a 3- / 4-deep ring
    "rows255": (lambda cus: (3, 255, 64, 128, -1), False),                      # the row-tile boundary: 3 or 6 tiles, identity order
    "rows256": (lambda cus: (3, 256, 64, 128, -1), False),
    "rows257": (lambda cus: (3, 257, 64, 128, -1), False),
    "bn128_30tiles": (lambda cus: (5, 300, 96, 384, -1), False),                # BN = 128, 30 tiles, 6 stages
    "bn256_ragged": (lambda cus: (2, 513, 160, 768, -1), False),                # BN = 256, 18 tiles, a third row tile of one row
    "turnover_k32": (lambda cus: (64, _turnover_mt(cus, 64, 3, 256, 1), 32, 384, -1), True),      # K shorter than the ring, XCD order
    "turnover_k96": (lambda cus: (64, _turnover_mt(cus, 64, 3, 256, 1), 96, 384, -1), True),
    "half_turnover": (lambda cus: (64, _turnover_mt(cus, 64, 2, 128, 2), 64, 512, 1), True),      # the 128-row form, two workgroups per CU
    "half_step_shape": (lambda cus: (36, 588, 32, 512, 1), False),              # ... without turn-over (the recurrent step's rows)
    "g14_identity": (lambda cus: (7, 257, 64, 256, -1), False),                 # G = 14 < CUs, not a multiple of 8, BN = 256
}

# Through ctx.gemm_split(half=2): the fp32-rows form, P = 1, no bias.  name -> (shape(cus) -> (Mt, K, N), turn-over premise)
ROWS_CASES = {"m%d_n%d" % (m, n): ((lambda cus, m=m, n=n: (m, 32, n)), False) for m in (1, 15, 16, 17, 255, 257) for n in (128, 256)}
ROWS_CASES["turnover_n384"] = (lambda cus: (256 * _cdiv(5 * cus, 2 * 3) + 37, 64, 384), True)
ROWS_CASES["turnover_n512"] = (lambda cus: (256 * _cdiv(5 * cus, 2 * 2) + 5, 32, 512), True)

# Through ctx.conv2d(k = 1) under DT_S3=2: (B, H, W) = (3, 13, 13) = 507 rows
CONV_COUT = (64, 85, 128, 200, 384, 512)
CONV_CIN = (32, 96)


def conv_turnover_batch(cus):
    """frames of 16 x 16 (one 256-row tile each) for the Cout = 85 turn-over case: ceil(2.5 CUs)"""
    return _cdiv(5 * cus, 2)


def table_k_values():
    ks = {f(256)[2] for f, _ in WINO_CASES.values()} | {f(256)[1] for f, _ in ROWS_CASES.values()} | set(CONV_CIN)
    return sorted(ks)


def all_tile_maps(cus):
    """(name, TileMap, turn-over premise) of every case of the table at a CU count"""
    out = []
    for name, (f, turn) in WINO_CASES.items():
        P, Mt, K, N, half = f(cus)
        out.append(("wino:" + name, TileMap(P, Mt, N, half, cus), turn))
    for name, (f, turn) in ROWS_CASES.items():
        Mt, K, N = f(cus)
        out.append(("rows:" + name, TileMap(1, Mt, N, 0, cus), turn))
    for cout in CONV_COUT:
        for half in (0, 1):
            out.append(("conv:%d_half%d" % (cout, half), TileMap(1, 3 * 13 * 13, cout, half, cus), False))
    out.append(("conv:turnover", TileMap(1, conv_turnover_batch(cus) * 256, 85, 0, cus), True))
    return out


def assert_turnover(tm):
    """the premise of a CU-sized case: more tiles than workgroups, and some workgroup runs at least three"""
    assert tm.tiles > tm.G, "%d tiles on %d workgroups: no workgroup takes a second tile" % (tm.tiles, tm.G)
    assert tm.max_turns() >= 3 and len(tm.sequence(0)) >= 3, "no workgroup runs three tiles (%d tiles, %d workgroups)" % (tm.tiles, tm.G)
