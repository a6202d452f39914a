"""float64 reference of the Winograd transforms around the batched GEMM (csrc/winograd.hip), in plain numpy and written differently from the
kernels: explicit Bt, At and G matrices (Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks"), applied as matrix products,
and a frame mosaic that is built by PAINTING the frames onto a canvas of zeros at the pitch (ph, pw) and slicing the tiles out of it --
no division maps a tile pixel back to a frame.

    V[p]  = (Bt d B)[xi][nu]            p = (ts+2) xi + nu,  d = the (ts+2)^2 window of a tile, rows / columns ts*t - 1 .. ts*t + ts
    Y     = At m A                      m[xi][nu] = M'[p],  ts x ts outputs per tile

Everything here is float64 unless a dtype is asked for; test_wino_transform_cpu.py checks it against a direct convolution."""
import numpy as np

BT = {
    2: np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64),
    4: np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
                dtype=np.float64),
    6: np.array([[1, 0, -5.25, 0, 5.25, 0, -1, 0], [0, 1, 1, -4.25, -4.25, 1, 1, 0], [0, -1, 1, 4.25, -4.25, -1, 1, 0],
                 [0, .5, .25, -2.5, -1.25, 2, 1, 0], [0, -.5, .25, 2.5, -1.25, -2, 1, 0], [0, 2, 4, -2.5, -5, .5, 1, 0],
                 [0, -2, 4, 2.5, -5, -.5, 1, 0], [0, -1, 0, 5.25, 0, -5.25, 0, 1]], dtype=np.float64),
}
AT = {
    2: np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64),
    4: np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64),
    6: np.array([[1, 1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, .5, -.5, 0], [0, 1, 1, 4, 4, .25, .25, 0], [0, 1, -1, 8, -8, .125, -.125, 0],
                 [0, 1, 1, 16, 16, .0625, .0625, 0], [0, 1, -1, 32, -32, .03125, -.03125, 1]], dtype=np.float64),
}
G = {
    2: np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64),
    4: np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                dtype=np.float64),
    6: np.array([[1, 0, 0], [-2 / 9, -2 / 9, -2 / 9], [-2 / 9, 2 / 9, -2 / 9], [1 / 90, 1 / 45, 2 / 45], [1 / 90, -1 / 45, 2 / 45],
                 [32 / 45, 16 / 45, 8 / 45], [32 / 45, -16 / 45, 8 / 45], [0, 0, 1]], dtype=np.float64),
}


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ geometry
def geometry(ts, B, H, W, pooled=False, mosaic=0):
    """The library's tile geometry rule.  One frame per virtual image (g = 1), or g x g frames at a pitch of one more than the frame (the
    next even number above it where the launch pools) when that takes at least 3 % fewer tiles per frame and the batch fills one mosaic;
    mosaic = DT_WINO_MOSAIC: 0 the rule, 1 never, 2..6 that g (unless a larger one wins by the rule)."""
    ph = H + 1 if not pooled else (H + 2 if H % 2 == 0 else H + 1)
    pw = W + 1 if not pooled else (W + 2 if W % 2 == 0 else W + 1)
    g, best = 1, float(_ceil_div(H, ts) * _ceil_div(W, ts))
    for k in range(2, 7):
        if mosaic == 1:
            break
        per_frame = _ceil_div(k * ph, ts) * _ceil_div(k * pw, ts) / float(k * k)
        if (per_frame < best * 0.97 and B >= k * k) or mosaic == k:
            g, best = k, per_frame
    if g == 1:
        th, tw, groups = _ceil_div(H, ts), _ceil_div(W, ts), B
    else:
        th, tw, groups = _ceil_div(g * ph, ts), _ceil_div(g * pw, ts), _ceil_div(B, g * g)
    Mt = groups * th * tw
    return dict(g=g, ph=ph, pw=pw, th=th, tw=tw, Mt=Mt, Mp=_ceil_div(Mt, 256) * 256)


def _groups(geo, B):
    return geo["Mt"] // (geo["th"] * geo["tw"])


def _frame_origins(geo, B):
    """(frame b, canvas group, row, column) of every frame's top-left pixel on its group's virtual image"""
    g = geo["g"]
    for b in range(B):
        grp, r = divmod(b, g * g)
        fy, fx = divmod(r, g)
        yield b, grp, fy * geo["ph"], fx * geo["pw"]


def windows(x, ts, geo):
    """x [B,H,W,C] -> the (ts+2) x (ts+2) input window of every tile, [Mt, ts+2, ts+2, C]; tile = (group, tile row, tile column)"""
    B, H, W, C = x.shape
    th, tw = geo["th"], geo["tw"]
    n_grp = _groups(geo, B)
    # one row / column of zeros in front ('same' padding), the tiles' extent behind
    canvas = np.zeros((n_grp, max(th * ts, geo["g"] * geo["ph"]) + 2, max(tw * ts, geo["g"] * geo["pw"]) + 2, C), dtype=np.float64)
    for b, grp, r0, c0 in _frame_origins(geo, B):
        canvas[grp, 1 + r0:1 + r0 + H, 1 + c0:1 + c0 + W] = x[b]
    d = np.empty((n_grp, th, tw, ts + 2, ts + 2, C), dtype=np.float64)
    for ty in range(th):
        for tx in range(tw):
            d[:, ty, tx] = canvas[:, ts * ty:ts * ty + ts + 2, ts * tx:ts * tx + ts + 2]
    return d.reshape(n_grp * th * tw, ts + 2, ts + 2, C)


def input_transform(x, ts, geo, dtype=np.float64, order=None):
    """V [P, Mt, C] = Bt d B of every tile's window"""
    d = windows(np.asarray(x, dtype=np.float64), ts, geo)
    if dtype == np.float64 and order is None:
        return _kron_apply(BT[ts], d.transpose(1, 2, 0, 3)).reshape((ts + 2) ** 2, d.shape[0], d.shape[3])
    v = sandwich(BT[ts], d.astype(dtype), dtype, order)         # [Mt, xi, nu, C]
    return np.ascontiguousarray(v.transpose(1, 2, 0, 3)).reshape((ts + 2) ** 2, d.shape[0], d.shape[3])


def _kron_apply(M, d):
    """M d Mt over the two leading axes of d [n, n, T, C] as ONE float64 matrix product with M (x) M -> [r, r, T, C]"""
    n, _, T, C = d.shape
    r = M.shape[0]
    return (np.kron(M, M) @ np.ascontiguousarray(d, dtype=np.float64).reshape(n * n, T * C)).reshape(r, r, T, C)


def sandwich(M, d, dtype=np.float64, order=None):
    """M d Mt over axes 1, 2 of d [T, n, n, C], every product and sum rounded to `dtype`, the sums taken in the order `order` (a permutation of
    range(n); None = ascending): the float32 evaluations in two orders that the exactness conditions are checked with"""
    n = M.shape[1]
    order = list(range(n)) if order is None else list(order)
    Md = M.astype(dtype)
    t = np.zeros((d.shape[0], M.shape[0], n, d.shape[3]), dtype=dtype)
    for k in order:                                                # rows: t[i][j] = sum_k M[i][k] d[k][j]
        t = (t + Md[None, :, k, None, None] * d[:, None, k, :, :]).astype(dtype)
    o = np.zeros((d.shape[0], M.shape[0], M.shape[0], d.shape[3]), dtype=dtype)
    for k in order:                                                # columns: o[i][l] = sum_k t[i][k] M[l][k]
        o = (o + t[:, :, k, None, :] * Md[None, None, :, k, None]).astype(dtype)
    return o


def tile_outputs(m, ts, dtype=np.float64, order=None):
    """M' [P, Mt, N] -> At m A per tile, [Mt, ts, ts, N]"""
    P, Mt, N = m.shape
    if dtype == np.float64 and order is None:
        return np.ascontiguousarray(_kron_apply(AT[ts], np.asarray(m).reshape(ts + 2, ts + 2, Mt, N)).transpose(2, 0, 1, 3))
    mm = np.asarray(m).reshape(ts + 2, ts + 2, Mt, N).transpose(2, 0, 1, 3).astype(dtype)
    return sandwich(AT[ts], mm, dtype, order)


def frames_from_tiles(y, ts, geo, B, H, W):
    """y [Mt, ts, ts, N] -> [B, H, W, N]: the tiles laid side by side give each group's virtual image, the frames are cut out of it"""
    th, tw = geo["th"], geo["tw"]
    n_grp = _groups(geo, B)
    N = y.shape[3]
    canvas = y.reshape(n_grp, th, tw, ts, ts, N).transpose(0, 1, 3, 2, 4, 5).reshape(n_grp, th * ts, tw * ts, N)
    out = np.empty((B, H, W, N), dtype=y.dtype)
    for b, grp, r0, c0 in _frame_origins(geo, B):
        out[b] = canvas[grp, r0:r0 + H, c0:c0 + W]
    return out


def border_case(H, W):
    """[H, W] ints: (h == 0) | (h == H-1) << 1 | (w == 0) << 2 | (w == W-1) << 3"""
    h, w = np.arange(H)[:, None], np.arange(W)[None, :]
    return (h == 0) * 1 + (h == H - 1) * 2 + (w == 0) * 4 + (w == W - 1) * 8


def leaky(v, slope):
    return np.where(v > 0, v, v * np.asarray(slope, dtype=v.dtype))


def output_transform(m, ts, geo, B, H, W, bias=None, bias16=None, slope=1.0, dtype=np.float64, order=None):
    """full-resolution output [B, H, W, N] = LeakyReLU(At m A + bias) (+ the border correction bias16[case] on border pixels: slope 1 only)"""
    y = frames_from_tiles(tile_outputs(m, ts, dtype, order), ts, geo, B, H, W)
    if bias is not None:
        y = (y + np.asarray(bias, dtype=dtype)).astype(dtype)
    y = leaky(y, slope).astype(dtype)
    if bias16 is not None:
        assert slope == 1.0
        k = border_case(H, W)
        corr = np.asarray(bias16, dtype=dtype)[k] * (k != 0)[:, :, None]
        y = (y + corr[None]).astype(dtype)
    return y


def pool2(y):
    """MaxPooling2D(2, 2): [B, H, W, N] -> [B, H//2, W//2, N]; the last row / column of an odd frame is dropped"""
    B, H, W, N = y.shape
    q = y[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, N)
    return q.max(axis=(2, 4))


def amax(y):
    return np.float32(np.abs(y).max()) if y.size else np.float32(0)


# ------------------------------------------------------------------------------------------------ ConvLSTM2D gate update
def gate_columns(U):
    """column of (gate k, hidden channel j) in the packed N = 4 U axis [j/32][gate][j%32]; gates i, f, c, o -> [4, U]"""
    j = np.arange(U)
    return np.stack([(j // 32) * 128 + k * 32 + j % 32 for k in range(4)])


def hard_sigmoid(z):
    return np.clip(z.dtype.type(0.2) * z + z.dtype.type(0.5), 0, 1).astype(z.dtype)      # Keras 2.x


def gate_update(z, c, dtype=np.float64):
    """z [..., 4U] packed pre-activations, c [..., U] -> (c_new, h), evaluated in `dtype`"""
    U = c.shape[-1]
    col = gate_columns(U)
    z = np.asarray(z, dtype=dtype)
    c = np.asarray(c, dtype=dtype)
    zi, zf, zc, zo = (z[..., col[k]] for k in range(4))
    c_new = (hard_sigmoid(zf) * c + hard_sigmoid(zi) * np.tanh(zc)).astype(dtype)
    h = (hard_sigmoid(zo) * np.tanh(c_new)).astype(dtype)
    return c_new, h


# ------------------------------------------------------------------------------------------------ weights and the direct form (self-check)
def filter_transform(w, ts):
    """w [3, 3, Cin, Cout] (HWIO) -> U [P, Cout, Cin] = G g Gt"""
    u = np.einsum("xa,abio,nb->xnoi", G[ts], np.asarray(w, dtype=np.float64), G[ts])
    return u.reshape((ts + 2) ** 2, w.shape[3], w.shape[2])


def conv_same(x, w):
    """direct 3x3 'same' stride-1 correlation (Keras Conv2D), float64: [B,H,W,Cin] x [3,3,Cin,Cout] -> [B,H,W,Cout]"""
    B, H, W, _ = x.shape
    xp = np.zeros((B, H + 2, W + 2, x.shape[3]), dtype=np.float64)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((B, H, W, w.shape[3]), dtype=np.float64)
    for a in range(3):
        for b in range(3):
            out += xp[:, a:a + H, b:b + W] @ np.asarray(w[a, b], dtype=np.float64)
    return out


# ------------------------------------------------------------------------------------------------ split layouts of V
def _blocked(v, Mp, fill):
    """[P, T, Mt, C] 16-bit words -> [P, T, C/16, Mp, 16], rows Mt .. Mp-1 = fill"""
    P, T, Mt, C = v.shape
    out = np.full((P, T, C // 16, Mp, 16), fill, dtype=np.uint16)
    out[:, :, :, :Mt] = v.reshape(P, T, Mt, C // 16, 16).transpose(0, 1, 3, 2, 4)
    return out


def _unblocked(words, Mt):
    P, T, CB, Mp, _ = words.shape
    return words[:, :, :, :Mt].transpose(0, 1, 3, 2, 4).reshape(P, T, Mt, CB * 16)


def bf16_round(x):
    """float32 -> bf16 bits, round to nearest even"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def pack_bf16x3(v, Mp, fill=0):
    """V [P, Mt, C] float32 -> three bf16 terms [P][3][C/16][Mp][16]: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), float32 arithmetic"""
    x = np.asarray(v, dtype=np.float32)
    h = bf16_round(x)
    r1 = (x - bf16_value(h)).astype(np.float32)
    m = bf16_round(r1)
    r2 = (r1 - bf16_value(m)).astype(np.float32)
    return _blocked(np.stack([h, m, bf16_round(r2)], axis=1), Mp, fill)


def unpack_bf16x3(words, Mt):
    t = bf16_value(_unblocked(words, Mt)).astype(np.float64)
    return t[:, 0] + t[:, 1] + t[:, 2]


def h2_rowfac(ts):
    """static part of the fp16 form's scale: a power of two per row of Bt d B that brings the row's absolute coefficient sum below 1"""
    return np.array([0.125 if i in (3, 4) else 0.0625 for i in range(ts + 2)], dtype=np.float64)


def h2_scale(ts, amax_in):
    """[P] float64: 2^(14 - floor(log2 amax)) * rowfac[xi] * rowfac[nu]"""
    e = np.frexp(np.float64(amax_in))[1] - 1            # floor(log2 amax), amax > 0 normal
    rf = h2_rowfac(ts)
    return (2.0 ** (14 - e)) * np.outer(rf, rf).reshape(-1)


def pack_f16x2(v, ts, amax_in, Mp, fill=0):
    """V [P, Mt, C] float32 -> two fp16 terms [P][2][C/16][Mp][16] of xs = V[p] * scale[p]: hi = f16(xs), lo = f16(xs - hi) (float32 arithmetic)"""
    xs = (np.asarray(v, dtype=np.float32) * h2_scale(ts, amax_in).astype(np.float32)[:, None, None]).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return _blocked(np.stack([hi.view(np.uint16), lo.view(np.uint16)], axis=1), Mp, fill)


def unpack_f16x2(words, ts, amax_in, Mt):
    t = _unblocked(words, Mt).view(np.float16).astype(np.float64)
    return (t[:, 0] + t[:, 1]) / h2_scale(ts, amax_in)[:, None, None]
