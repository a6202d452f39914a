"""GPU suite: the fp32 implicit-GEMM kernel (csrc/conv_igemm.hip) ALONE, through its production launcher, at the smallest shapes at which each of
its mechanisms can fail -- against the integer / float64 references of tests/conv_igemm_cases.py, bit for bit wherever the operands allow it.

The layer tests reach this kernel through dt_conv2d / dt_convlstm_step on dense random tensors at 2e-5 relative.  Here the test entry
dt_conv_igemm (Context.conv_igemm) hands the launcher caller views with strides, a tile configuration, a split count and a workgroup cap, and
reports WHICH INSTANCE ran on what grid (the launcher's own plan_conv_igemm); every case asserts that before it looks at a value, so a moved
threshold fails here instead of moving coverage.  Every output buffer is pre-filled with a NaN bit pattern -- columns N .. ld-1, the columns in
front of a column offset and a guard band of rows behind M included -- and every word the kernel does not own must keep it; the input's unused
columns Cin .. in_ld-1 and the gap between frames hold NaN, so one word read from there shows in a sum.  Families A / As / H are compared with
array_equal and a failure names the tile, workgroup, turn and split ranges (Schedule.locate); family D is held to d_bar().

The 35 instances launch_conv_igemm dispatches -> the cases that run them (conv_igemm_cases.py; the CPU suite asserts the table reaches all 35):
  plain 3x3 x 5 cfgs                R_3x3_*, C_3x3_*, K_3x3_*, S_3x3_*                 production: every 3x3 layer the other forms decline, xproj
  plain 1x1 x 5 cfgs (persistent)   R_1x1_*, C_1x1_*, K_1x1_*, S_1x1_*, P1..P6, Dh     production: 1x1 layers, all fp32 Winograd GEMMs, Dense head
  pool 3x3 / pool 1x1 x 5 cfgs      Q_pool_*                                           production: pooled layers (3x3); pool 1x1: no layer today
  pool_both 3x3 x 5 cfgs            Q_both_*                                           production: conv_13
  s2d 1x1 x 5 cfgs                  Q_s2d_*                                            production: conv_21
  gates 3x3 128x128 / 256x256, 1x1  G_3x3_*, G_3x3_256_* (U % 64 == 0), G_1x1_*        production: the ConvLSTM step (3x3); gates 1x1: none today
  partial 3x3 / 1x1                 SK_*                                               production: small-batch layers (CF_SPLITK)
Production picks 128x64 only for Cout <= 64 and 64x128 only for a handful of Winograd tiles; the entry hands every configuration to every kind,
which the launcher accepts.  Nothing turned out unreachable through the entry, with one correction to the issue's premise: a layer's weights
are padded to a multiple of 256 rows (load_conv_layer), so N = 257 runs the 256x256 tile itself; the 256x256 -> 256x128 fallback needs weight
rows that are NOT a multiple of 256 (the tracker's layers, Winograd U) and is reached with npad = 384 (C_*_N257_npad384) and by the gate cases
at U = 32 / 96.

Findings.  P6 (P6_raw_publish*): the raw fast epilogue of the persistent instances returned before the lane's running maximum was updated, so a
bias-less linear launch with amax_out set published 0; the kernel now takes the general epilogue when a slot is passed (no production launch
did both).  The launcher now refuses ORD_QUAD with odd H or W (test_launcher_refusals).

Measured on an MI355X (this file, `pytest -s`), error / bar:
  family D  max |got - ref64| / (sum |a||w| + |b|), rms in brackets:
    plain 3x3 128x128             K =  288: 5.8e-07 [8.1e-08] of 3.5e-05    K = 576: 7.4e-07 [8.5e-08] of 6.9e-05    K = 864: 7.4e-07 [8.7e-08] of 1.0e-04
    plain 1x1 128x128 persistent  K =   32: 4.2e-07 [6.0e-08] of 4.2e-06    K =  64: 5.3e-07 [7.0e-08] of 8.0e-06    K =  96: 5.0e-07 [7.4e-08] of 1.2e-05
    partial 3x3 / 1x1 (+ reduce)  SK_*_D: printed by the cases (added after the first measurement; the same kernel body and K lengths as above)
    (the maximum is about 10 x 2^-24 whatever K is, the rms about 1.4 x 2^-24: the bound's K is far from reached on random signs)
  sigmoid head (Dh)  max |got - sigmoid64| = 5.5e-08 (bar 2^-21 = 4.77e-07)
  gates  max |c - ref| / (atol + rtol |ref|) = 0.0022, the same for h (bar 1), over all 24 gate cases"""
import numpy as np
import pytest
import torch

import conv_igemm_cases as cc
import mi355_dt

pytestmark = pytest.mark.gpu

S32 = np.uint32(cc.SENTINEL32)
GUARD_ROWS = 8
DT_ERR_ARG = 1      # include/mi355_dt.h


@pytest.fixture(autouse=True)
def _policy_env(monkeypatch):
    for k in ("DT_PIN", "DT_CONV_CFG"):
        monkeypatch.delenv(k, raising=False)


class _Rows(object):
    """`rows` rows of `ld` words pre-filled with the sentinel, a guard band of rows behind them; the kernel owns columns [off, off + cols)"""

    def __init__(self, ctx, rows, cols, ld, off=0, init=None):
        assert off + cols <= ld
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.t = torch.full(((rows + GUARD_ROWS) * ld,), int(S32.view(np.int32)), dtype=torch.int32, device=ctx.device)
        self.view = self.t.view(torch.float32)[off:].as_strided((rows, cols), (ld, 1))
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).to(ctx.device))

    def read(self, what):
        """the owned block as float32 [rows, cols]; fails if any other word lost the sentinel"""
        torch.cuda.synchronize()
        words = self.t.cpu().numpy().view(np.uint32).reshape(self.rows + GUARD_ROWS, self.ld)
        mask = np.ones(words.shape, dtype=bool)
        mask[:self.rows, self.off:self.off + self.cols] = False
        stray = np.argwhere((words != S32) & mask)
        assert stray.size == 0, "%s: %d words outside what the kernel owns were written (first: row %d column %d of ld %d; %d rows, columns %d..%d owned)" % (
            what, len(stray), stray[0][0], stray[0][1], self.ld, self.rows, self.off, self.off + self.cols - 1)
        return words[:self.rows, self.off:self.off + self.cols].view(np.float32).copy()


def _upload_x(ctx, k, x):
    """the input view: pixel stride in_ld, frames in_gap floats further apart, NaN in every word that is not a channel of a pixel"""
    if k["P"] > 1:
        return torch.from_numpy(x).to(ctx.device)
    B, H, W, Cin = x.shape
    ld = k["in_ld"]
    bs = H * W * ld + k["in_gap"]
    buf = torch.full((B * bs + 64,), float("nan"), dtype=torch.float32, device=ctx.device)
    view = buf.as_strided((B, H, W, Cin), (bs, W * ld, ld, 1))
    view.copy_(torch.from_numpy(x).to(ctx.device))
    return view


def _M(k):
    return k["W"] if k["P"] > 1 else k["B"] * k["H"] * k["W"]


def _cus(ctx):
    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def _run(ctx, k, o=None):
    """runs the case; returns (info, outputs dict of float32 arrays, published max or None)"""
    o = o or cc.operands(k)
    M, N, P = _M(k), k["N"], max(k["P"], 1)
    kind = k["kind"]
    x = _upload_x(ctx, k, o["x"])
    rows = {"plain": M, "pool": M // 4, "pool_both": M, "s2d": M // 4, "gates": M}[kind] * P
    cols = {"s2d": 4 * N, "gates": N // 4}.get(kind, N)
    out = _Rows(ctx, rows, cols, cols + k["out_extra"], k["col_off"])
    kw, bufs = {}, {"out": out}
    if kind == "pool_both":
        bufs["out2"] = _Rows(ctx, M // 4, N, N + k["out2_extra"])
        kw["out2"] = bufs["out2"].view
    if kind == "gates":
        bufs["cstate"] = _Rows(ctx, M, N // 4, N // 4 + k["c_extra"], init=o["cstate"])
        xp = torch.full((M, N + k["xp_extra"]), float("nan"), dtype=torch.float32, device=ctx.device)
        xp[:, :N] = torch.from_numpy(o["xproj"]).to(ctx.device)
        kw["xproj"], kw["cstate"] = xp[:, :N], bufs["cstate"].view
    if P > 1:
        kw["wt"] = torch.from_numpy(o["w"]).to(ctx.device)
        oview = out.view.as_strided((P, M, cols), (M * out.ld, out.ld, 1))
    else:
        kw["kernel"], kw["bias"] = o["w"], o["bias"]
        oview = out.view
    info = ctx.conv_igemm(x, oview, k["ks"], kind=kind, cfg=k["cfg"], slope=k["slope"], act=k["act"], ksplit=k["ksplit"], npad=k["npad"],
                          publish=k["publish"], wg_cap=k["wg_cap"], **kw)
    want = cc.expected_info(k, _cus(ctx))
    assert info == want, "%s: ran %r, the case is about %r" % (k["name"], info, want)
    got = {n: b.read("%s %s" % (k["name"], n)) for n, b in bufs.items()}
    return info, got, (ctx.amax_read(57) if k["publish"] else None)


def _where(k, info, z, m, n):
    s = cc.Schedule(_M(k), k["N"], info["BM"], info["BN"], k["P"], cc.tile_gn_of(k["ks"], k["kind"]), info["grid_x"])
    return s.locate(z, m, n, k["ks"] ** 2 * k["Cin"] // 32, max(k["ksplit"], 1))


def _assert_equal(k, info, got, want, what, row_to_m=lambda r: r, col_to_n=lambda c: c):
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (k["name"], what, got.shape, want.shape)
    if np.array_equal(got, want):      # (zeros compare equal whatever their sign; no NaN is expected)
        return
    bad = np.argwhere(got != want)
    r, c = (int(v) for v in bad[0])
    M = _M(k)
    m = row_to_m(r)
    pytest.fail("%s %s: %d of %d values differ; first at row %d column %d: got %r expected %r; computed at %r" % (
        k["name"], what, len(bad), got.size, r, c, float(got[r, c]), float(want[r, c]), _where(k, info, m // M if k["P"] > 1 else 0, m % M, col_to_n(c))))


def _expected_plain(k, o):
    """[P M, N] float32 for the exact families: the activation of the exact pre-activation"""
    Z = cc.preact(k, o)
    return cc.act32(Z, o["bias"], k["slope"]).reshape(-1, k["N"])


_D_SEEN, _G_SEEN, _SIG_SEEN = {}, {}, {}


def _check_case(ctx, k):
    o = cc.operands(k)
    info, got, amax = _run(ctx, k, o)
    N, kind = k["N"], k["kind"]
    B, H, W = k["B"], k["H"], k["W"]
    if k["fam"] == "D":
        ref = cc.preact(k, o)[0] + o["bias"].astype(np.float64)
        scale = cc.conv_abs(o["x"], o["w"], o["bias"]).reshape(-1, N)
        assert k["slope"] == 1.0 and kind == "plain"
        e = np.abs(got["out"].astype(np.float64) - ref) / scale
        bar = cc.d_bar(k["ks"] ** 2 * k["Cin"], k["ksplit"])
        _D_SEEN[k["name"]] = (float(e.max()), float(np.sqrt(np.mean(e * e))), bar)
        print("%s: family D max %.3g rms %.3g of bar %.3g (%s)" % (k["name"], e.max(), np.sqrt(np.mean(e * e)), bar, cc.instance_of(k)))
        assert e.max() <= bar, (k["name"], float(e.max()), bar, _where(k, info, 0, *(int(v) for v in np.unravel_index(e.argmax(), e.shape))))
        return
    if k["act"] == 1:
        ref = cc.sigmoid64(cc.preact(k, o)[0], o["bias"])
        e = np.abs(got["out"].astype(np.float64) - ref)
        _SIG_SEEN[k["name"]] = float(e.max())
        print("%s: sigmoid max abs error %.3g of bar %.3g" % (k["name"], e.max(), cc.SIGMOID_BAR))
        assert e.max() <= cc.SIGMOID_BAR, (k["name"], float(e.max()), _where(k, info, 0, *(int(v) for v in np.unravel_index(e.argmax(), e.shape))))
        return
    if kind == "gates":
        U = N // 4
        z_keras = cc.preact(k, o)[0] + o["xproj"].astype(np.int64)[:, np.argsort(cc.gate_columns(U))]      # packed xproj column n' -> Keras column n_map[n']
        c_ref, h_ref = cc.gate_update(z_keras, o["cstate"])
        worst = {}
        for name, g, r in (("c", got["cstate"], c_ref), ("h", got["out"], h_ref)):
            e = np.abs(g.astype(np.float64) - r) / (cc.GATE_ATOL + cc.GATE_RTOL * np.abs(r))
            worst[name] = float(e.max())
            i = tuple(int(v) for v in np.unravel_index(e.argmax(), e.shape))
            assert e.max() <= 1.0, (k["name"], name, float(g[i]), float(r[i]), "row %d hidden channel %d" % i, _where(k, info, 0, i[0], (i[1] // 32) * 128 + i[1] % 32))
        _G_SEEN[k["name"]] = worst
        print("%s: gates c %.3g h %.3g of the bar" % (k["name"], worst["c"], worst["h"]))
        return
    if kind == "plain":
        want = _expected_plain(k, o)
        _assert_equal(k, info, got["out"], want, "out")
        stored = want
    else:
        v_quad = cc.act32(cc.preact(k, o)[0], o["bias"], k["slope"])      # [M, N], quad row order
        bq, hq, wq = cc.quad_rows(B, H, W)
        v = np.empty((B, H, W, N), np.float32)
        v[bq, hq, wq] = v_quad
        pooled = cc.maxpool2(v).reshape(-1, N)
        if kind == "pool":
            _assert_equal(k, info, got["out"], pooled, "pooled", row_to_m=lambda r: 4 * r)
            stored = pooled
        elif kind == "pool_both":
            lin_to_quad = np.empty(B * H * W, np.int64)
            lin_to_quad[(bq * H + hq) * W + wq] = np.arange(B * H * W)
            _assert_equal(k, info, got["out"], v.reshape(-1, N), "unpooled", row_to_m=lambda r: int(lin_to_quad[r]))
            _assert_equal(k, info, got["out2"], pooled, "pooled", row_to_m=lambda r: 4 * r)
            stored = pooled
        else:
            s2d = cc.space_to_depth2(v).reshape(-1, 4 * N)
            _assert_equal(k, info, got["out"], s2d, "space_to_depth", row_to_m=lambda r: 4 * r, col_to_n=lambda c: c % N)
            stored = s2d
    if k["publish"]:
        assert amax == np.abs(stored).max(), "%s: published max |x| %r, the stored tensor's is %r" % (k["name"], float(amax), float(np.abs(stored).max()))


def _param(group):
    return pytest.mark.parametrize("name", cc.case_ids(group))


@_param("R")
def test_row_edge(ctx, name):
    _check_case(ctx, cc.CASES[name])


@_param("C")
def test_column_edge(ctx, name):
    _check_case(ctx, cc.CASES[name])


@_param("K")
def test_chunk_order(ctx, name):
    _check_case(ctx, cc.CASES[name])


@_param("S")
def test_strides(ctx, name):
    _check_case(ctx, cc.CASES[name])


@_param("P")
def test_persistent_walk(ctx, name):
    k = cc.CASES[name]
    want = cc.expected_info(k, _cus(ctx))
    assert want["persistent"] and want["total"] > want["grid_x"] == k["wg_cap"], name      # some workgroup takes a second tile
    _check_case(ctx, k)


@_param("P6")
def test_published_maximum_of_a_persistent_launch(ctx, name):
    k = cc.CASES[name]
    assert k["publish"] and cc.expected_info(k, _cus(ctx))["persistent"]
    _check_case(ctx, k)


@pytest.mark.parametrize("cfg", ["128x128", "256x256"])
def test_production_grid_walks_three_tiles(ctx, cfg):
    """P5: no cap -- the launcher's own persistent grid (2 x CUs workgroups of 4 waves, 1 x CUs of 16), more than twice as many tiles, K = 32.
    The reference is the float64 product on the device (family A: exact)."""
    cus = _cus(ctx)
    BM, BN, threads = cc.CFG_TILES[cfg]
    slots = cus * (1 if threads > 256 else 2) // 8 * 8
    P, N = 5, BN + 1                                     # two column tiles, the second one column wide
    ntm = 2 * slots // (2 * P) + 1
    Mt = ntm * BM - 3
    k = dict(name="P5_" + cfg, ks=1, B=1, H=1, W=Mt, Cin=32, N=N, kind="plain", cfg=cfg, fam="A", P=P, bias=False, slope=1.0, act=0, ksplit=0, npad=0,
             wg_cap=0, publish=False, in_ld=32, in_gap=0, out_extra=4 - N % 4, col_off=0, seed=77)
    want = cc.expected_info(k, cus)
    assert want["grid_x"] == slots and want["total"] > 2 * slots, "the premise: a capped grid on which some workgroup runs three tiles (%r)" % (want,)
    rs = np.random.RandomState(77)
    o = {"x": rs.randint(-8, 9, (P, Mt, 32)).astype(np.float32), "w": rs.randint(-8, 9, (P, N, 32)).astype(np.float32), "bias": None}
    info, got, _ = _run(ctx, k, o)
    assert info["grid_x"] == slots < info["total"] and -(-info["total"] // info["grid_x"]) >= 3, info
    ref = torch.bmm(torch.from_numpy(o["x"]).to(ctx.device).double(), torch.from_numpy(o["w"]).to(ctx.device).double().transpose(1, 2)).float().cpu().numpy()
    _assert_equal(k, info, got["out"], ref.reshape(-1, N), "out")


@_param("Dh")
def test_dense_sigmoid_head(ctx, name):
    _check_case(ctx, cc.CASES[name])


@_param("Q")
def test_quad_epilogues(ctx, name):
    _check_case(ctx, cc.CASES[name])


@_param("SK")
def test_split_k(ctx, name):
    k = cc.CASES[name]
    _check_case(ctx, k)


@_param("G")
def test_gates(ctx, name):
    _check_case(ctx, cc.CASES[name])


def test_launcher_refusals(ctx):
    """DT_ERR_ARG and no launch: the outputs keep their sentinel (the exception leaves before they are read, so read them here)"""
    for over in (dict(kind="pool", B=1, H=3, W=4, N=72), dict(kind="s2d", ks=1, B=1, H=4, W=3, N=72), dict(kind="pool_both", B=1, H=5, W=5, N=72, out2_extra=0),
                 dict(Cin=48), dict(ks=1, B=2, H=4, W=4, in_gap=64), dict(ksplit=10), dict(ks=1, ksplit=2)):
        k = dict(cc.CASES["R_3x3_128x128_M128"], name="refused", publish=False, out2_extra=0)
        k.update(over)
        rs = np.random.RandomState(3)
        x = rs.randint(-8, 9, (k["B"], k["H"], k["W"], k["Cin"])).astype(np.float32)
        w = rs.randint(-8, 9, (k["ks"], k["ks"], k["Cin"], k["N"])).astype(np.float32)
        xv = _upload_x(ctx, dict(k, in_ld=k["Cin"]), x)
        M = k["B"] * k["H"] * k["W"]
        out = _Rows(ctx, M, 4 * k["N"], 4 * k["N"])
        out2 = _Rows(ctx, M, k["N"], k["N"]) if k["kind"] == "pool_both" else None
        with pytest.raises(mi355_dt.NativeError, match=r"dt_conv_igemm: (the launcher refuses|unsupported arguments)") as ei:
            ctx.conv_igemm(xv, out.view[:, :(4 * k["N"] if k["kind"] == "s2d" else k["N"])], k["ks"], kernel=w, bias=None, kind=k["kind"], cfg=k["cfg"],
                           ksplit=k["ksplit"], out2=None if out2 is None else out2.view)
        assert "dt_conv_igemm failed (%d)" % DT_ERR_ARG in str(ei.value), (over, str(ei.value))
        torch.cuda.synchronize()
        assert bool((out.t == int(S32.view(np.int32))).all()) and (out2 is None or bool((out2.t == int(S32.view(np.int32))).all())), over


def test_every_instance_was_asserted_from_h_info():
    """_run asserts h_info == expected_info for every case it runs and the table's expected instances are all 35 (the CPU suite proves the same on the
    table alone): with every case above passed, every instance has run under its own name"""
    assert sorted({cc.instance_of(k) for k in cc.CASES.values()}) == cc.ALL_INSTANCES
