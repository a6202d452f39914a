"""GPU suite: the split GEMM (csrc/wino_gemm_s3.hip) at SMALL shapes chosen for its tile loop, its LDS ring and its edges, with operands
for which the expected result is bit-exact -- a failure names an element, its tile, the workgroup and the turn that computed it.

The kernel is persistent: min(tiles, CUs) workgroups (2 x CUs in the 128-row form) walk the tiles with stride gridDim.x through a ring
of 2, 3 or 4 LDS stages of 16 k each, the next tile's first stages in flight during a tile's epilogue.  From its second tile on a
workgroup runs code its first tile never runs (new DMA sources while stages are in flight, `drain`, the second accumulator clear), and
with K = 32 (two stages) the prologue of a 3- or 4-deep ring already crosses into the next tile or runs out of stages.  The other
tests reach the kernel at bench-sized shapes with statistical bars, or through the F(6x6) transforms at 2e-4, where a `lo` term dropped
on part of a tile (2^-11 per element) passes.

Operands (tests/gemm_split_cases.py; the claims are proven on the numpy model in tests/test_gemm_split_cases_cpu.py):
  A  integers in [-8, 8]: expected = the integer product, bit for bit, in both operand forms;
  B  n (1 + 2^-13): expected = float32(float64 product), bit for bit; a lost cross product moves every element by >= 1024 places;
  D  13 binades, heavy tails: error relative to sum |v||u| (+ |b|) at the project's absolute bars, rms < 1.5 x 2^-24 and max < 32 x 2^-24
     (the only family that sees the three smallest products of the bf16 form).  Measured on the MI355X over all cases below, in units of
     2^-24: f16x2 rms <= 1.03, max <= 10.9; bf16x3 rms <= 1.05, max <= 12.1 (the numpy model: 0.87 / 5.8 -- the MFMA rounds inside a block).
Reference: float64 torch.bmm on the device (checked against numpy on the host in test_reference_against_numpy).

Every case runs in both operand forms (nt = 2: two fp16 terms, nt = 3: three bf16 terms) and asserts from the profile which tile form
ran.  Sizes marked CU in the case table come from the device's multi_processor_count; such a test asserts its premise (more tiles than
workgroups, some workgroup runs three) and FAILS -- it does not skip -- where the premise does not hold.

Instances (BN, operand kind, rows per tile, NT) and the cases that run them -- each for NT = 2 and NT = 3:
  BN 128, Winograd operands, 256 rows   one_row_k32, rows255 / 256 / 257, bn128_30tiles, turnover_k32 / k96
  BN 256, Winograd operands, 256 rows   bn256_ragged, g14_identity
  BN 256, Winograd operands, 128 rows   half_turnover, half_step_shape
  BN 128, fp32 rows, 256 rows           rows m*_n128, turnover_n384; conv Cout 64 / 85 / 128 / 200 / 384 (+ bias, LeakyReLU), conv turn-over
  BN 256, fp32 rows, 256 rows           rows m*_n256, turnover_n512; conv Cout 512 under DT_S3_HALF=0
  BN 256, fp32 rows, 128 rows           conv Cout 512 under DT_S3_HALF=1 (the only way to these two instances)

Not reachable through the entry points, hence untested: a_ld > K (dt_gemm_split and dt_conv2d hand over dense rows), ldc > N (dense
outputs), and an odd K / 16 without the bias stage (both entries require K % 32 == 0; the bf16 form's bias stage makes the stage
count odd, which the conv cases under DT_S3_H2=0 cover)."""
import numpy as np
import pytest
import torch

import gemm_split_cases as gc

pytestmark = pytest.mark.gpu

NT_IDS = {2: "f16x2", 3: "bf16x3"}
_cache = {}      # one entry: the operands and float64 reference of the last (kind, case, family) -- shared by the two operand forms


def _cus(ctx):
    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def _seed(*key):
    return sum(ord(c) * (i + 1) for i, c in enumerate("/".join(str(k) for k in key))) % (2 ** 31)


def _shared(key, make):
    if _cache.get("key") != key:
        _cache.clear()
        _cache.update(key=key, value=make())
    return _cache["value"]


def _bmm64(v, u):
    """float64 product and sum |v||u| on the device, plane by plane (bounded memory)"""
    ref = torch.empty(v.shape[0], v.shape[1], u.shape[1], dtype=torch.float64, device=v.device)
    scale = torch.empty_like(ref)
    for p in range(v.shape[0]):
        v64, u64 = v[p].double(), u[p].double()
        ref[p] = v64 @ u64.t()
        scale[p] = v64.abs() @ u64.abs().t()
    return ref, scale


def _operands(ctx, family, P, Mt, K, N, key):
    def make():
        v, u = gc.FAMILIES[family](P, Mt, K, N, _seed(*key))
        v, u = torch.from_numpy(v).to(ctx.device), torch.from_numpy(u).to(ctx.device)
        return (v, u) + _bmm64(v, u)
    return _shared(key, make)


def _assert_exact(got, ref64, tm, what):
    """got == float32(ref64), bit for bit; on a mismatch: how many, and the first one with its tile, workgroup and turn"""
    want = ref64.float()
    assert torch.equal(want.double(), ref64) or what[0] != "A", "family A's reference is not an integer product"
    bad = got.view(torch.int32) != want.view(torch.int32)
    n_bad = int(bad.sum())
    if n_bad:
        idx = torch.nonzero(bad.reshape(tm.P, -1, got.shape[-1]))[0].tolist()
        p, m, n = idx
        L, w, turn = tm.locate(p, m, n)
        pytest.fail("%s: %d of %d elements wrong; first at (p, m, n) = (%d, %d, %d): got %r expected %r -- tile %d of %d, workgroup %d of %d, turn %d"
                    % (what, n_bad, bad.numel(), p, m, n, float(got.reshape(tm.P, -1, got.shape[-1])[p, m, n]),
                       float(want.reshape(tm.P, -1, got.shape[-1])[p, m, n]), L, tm.tiles, w, tm.G, turn))


def _assert_bars(got, ref64, scale64, what):
    e = (got.double() - ref64).abs() / scale64
    rms, mx = float(e.pow(2).mean().sqrt()), float(e.max())
    print("gemm_split_edges D %s: rms %.3f max %.3f (x 2^-24; bars 1.5 / 32)" % (what, rms * 2.0 ** 24, mx * 2.0 ** 24))
    assert bool(torch.isfinite(got).all())
    assert rms < gc.D_RMS_BAR and mx < gc.D_MAX_BAR, (what, rms * 2.0 ** 24, mx * 2.0 ** 24)


def _gemm(ctx, v, u, half, nt, tm):
    ctx.profile_reset(); ctx.profile_enable(True)
    got = ctx.gemm_split(v, u, half=half, nt=nt)
    ctx.profile_enable(False)
    other = "s3_tile:256" if tm.half_form else "s3_tile:128x2"
    assert ctx.profile_read("conv_gemm_s3")["launches"] == 1
    assert ctx.profile_read(tm.tag())["launches"] == 1 and ctx.profile_read(other)["launches"] == 0, (tm.tag(), ctx.profile_names())
    return got


def _judge(family, got, ref, scale, tm, what):
    if family == "D":
        _assert_bars(got, ref, scale, what)
    else:
        _assert_exact(got, ref, tm, family + " " + what)


# ------------------------------------------------------------------------------------------------ the Winograd-operand instances
@pytest.mark.parametrize("family", ["A", "B", "D"])
@pytest.mark.parametrize("case", list(gc.WINO_CASES))
@pytest.mark.parametrize("nt", [2, 3], ids=["f16x2", "bf16x3"])
def test_winograd_operand_form(ctx, case, family, nt):
    shape, turnover = gc.WINO_CASES[case]
    P, Mt, K, N, half = shape(_cus(ctx))
    tm = gc.TileMap(P, Mt, N, half, _cus(ctx))
    assert tm.half_form == (half == 1)
    if turnover:
        gc.assert_turnover(tm)
        assert tm.xcd_order, "G = %d is no multiple of 8: this case is about the XCD order" % tm.G
    if case == "g14_identity":
        assert tm.G == 14 and not tm.xcd_order and tm.G < _cus(ctx)
    v, u, ref, scale = _operands(ctx, family, P, Mt, K, N, ("wino", case, family))
    got = _gemm(ctx, v, u, half, nt, tm)
    _judge(family, got, ref, scale, tm, "%s %s P=%d Mt=%d K=%d N=%d half=%d" % (case, NT_IDS[nt], P, Mt, K, N, half))


# ------------------------------------------------------------------------------------------------ the fp32-rows form, no bias
@pytest.mark.parametrize("family", ["A", "B", "D"])
@pytest.mark.parametrize("case", list(gc.ROWS_CASES))
@pytest.mark.parametrize("nt", [2, 3], ids=["f16x2", "bf16x3"])
def test_rows_form(ctx, case, family, nt):
    shape, turnover = gc.ROWS_CASES[case]
    Mt, K, N = shape(_cus(ctx))
    tm = gc.TileMap(1, Mt, N, 0, _cus(ctx))
    assert not tm.half_form      # (the launcher's own choice at these sizes; the 128-row x rows instances: the conv cases below)
    if turnover:
        gc.assert_turnover(tm)
    v, u, ref, scale = _operands(ctx, family, 1, Mt, K, N, ("rows", case, family))
    got = _gemm(ctx, v, u, 2, nt, tm)
    _judge(family, got, ref, scale, tm, "rows %s %s Mt=%d K=%d N=%d" % (case, NT_IDS[nt], Mt, K, N))


def test_reference_against_numpy(ctx):
    """the device's float64 product is the host's: exactly on A and B (every float64 partial sum is exact), to float64 rounding on D"""
    P, Mt, K, N, _ = gc.WINO_CASES["rows257"][0](_cus(ctx))
    for family in "ABD":
        v, u = gc.FAMILIES[family](P, Mt, K, N, 5)
        ref, scale = _bmm64(torch.from_numpy(v).to(ctx.device), torch.from_numpy(u).to(ctx.device))
        href, hscale = gc.reference(v, u)
        if family == "D":
            assert np.abs(ref.cpu().numpy() - href).max() <= 1e-13 * hscale.max() and np.allclose(scale.cpu().numpy(), hscale, rtol=1e-13, atol=0)
        else:
            assert np.array_equal(ref.cpu().numpy(), href) and np.array_equal(scale.cpu().numpy(), hscale)


# ------------------------------------------------------------------------------------------------ the rows form as the 1x1 layers use it
def _conv_env(monkeypatch, h2, half):
    for k in ("DT_PIN", "DT_WINO", "DT_S3_1X1", "DT_S3_1X1_MINK", "DT_S3_1X1_MINROWS", "DT_S3_MINROWS", "DT_H2_MINFRAMES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DT_S3", "2")
    monkeypatch.setenv("DT_S3_H2", h2)
    monkeypatch.setenv("DT_S3_HALF", half)


def _conv_operands(ctx, family, B, H, W, Cin, Cout, key):
    """x [B, H, W, Cin] on the device, w [1, 1, Cin, Cout] and b [Cout] on the host, float64 reference and scale [1, B H W, Cout]"""
    def make():
        M = B * H * W
        v, u = gc.FAMILIES[family](1, M, Cin, Cout, _seed(*key))
        rs = np.random.RandomState(_seed(*key) ^ 0x5bd1)
        b = rs.randint(-100, 101, Cout).astype(np.float32) if family == "A" else rs.randn(Cout).astype(np.float32)
        slope = np.float32(0.5 if family == "A" else 0.1)
        vd, ud = torch.from_numpy(v).to(ctx.device), torch.from_numpy(u).to(ctx.device)
        ref, scale = _bmm64(vd, ud)
        b64 = torch.from_numpy(b).to(ctx.device).double()
        ref = ref + b64
        ref = torch.where(ref > 0, ref, ref * float(slope))      # (float64 of the float32 slope: the number the kernel multiplies by)
        w = np.ascontiguousarray(u[0].T).reshape(1, 1, Cin, Cout)
        return vd.reshape(B, H, W, Cin), w, b, float(slope), ref, scale + b64.abs()
    return _shared(key, make)


def _conv(ctx, x, w, b, slope, h2):
    ctx.profile_reset(); ctx.profile_enable(True)
    got = ctx.conv2d(x, w, b, leaky_slope=slope, pool=0)
    ctx.profile_enable(False)
    form, other = ("s3_form:f16x2", "s3_form:bf16x3") if h2 == "1" else ("s3_form:bf16x3", "s3_form:f16x2")
    assert ctx.profile_read("conv_gemm_s3")["launches"] == 1 and ctx.profile_read("conv_igemm")["launches"] == 0
    assert ctx.profile_read(form)["launches"] == 1 and ctx.profile_read(other)["launches"] == 0, ctx.profile_names()
    return got.reshape(1, -1, got.shape[-1])


# DT_S3_HALF only matters where Cout % 256 == 0: Cout = 512 runs under both settings, the others under 0
CONV_SHAPES = [(cout, cin, half) for cout in gc.CONV_COUT for cin in gc.CONV_CIN for half in (("0", "1") if cout % 256 == 0 else ("0",))]


@pytest.mark.parametrize("cout,cin,half", CONV_SHAPES)
@pytest.mark.parametrize("h2", ["1", "0"], ids=["f16x2", "bf16x3"])
def test_conv1x1_integers_with_bias_and_leaky(ctx, monkeypatch, cout, cin, half, h2):
    """integer x, w and bias, slope 0.5: the float64 reference bit for bit.  Under DT_S3_H2=0 the bias rides as an extra -- odd -- K stage."""
    _conv_env(monkeypatch, h2, half)
    B, H, W = 3, 13, 13
    tm = gc.TileMap(1, B * H * W, cout, int(half), _cus(ctx))
    assert tm.half_form == (half == "1" and cout % 256 == 0)
    x, w, b, slope, ref, _ = _conv_operands(ctx, "A", B, H, W, cin, cout, ("conv", cout, cin, "A"))
    got = _conv(ctx, x, w, b, slope, h2)
    _assert_exact(got, ref, tm, "A conv1x1 %s Cin=%d Cout=%d DT_S3_HALF=%s" % (NT_IDS[2 if h2 == "1" else 3], cin, cout, half))


@pytest.mark.parametrize("h2", ["1", "0"], ids=["f16x2", "bf16x3"])
def test_conv1x1_turnover_ragged_n(ctx, monkeypatch, h2):
    """conv_23's shape class (85 outputs, 85-float rows) with ceil(2.5 CUs) row tiles: every workgroup's later tiles, clipped columns"""
    _conv_env(monkeypatch, h2, "0")
    B, H, W, cin, cout = gc.conv_turnover_batch(_cus(ctx)), 16, 16, 32, 85
    tm = gc.TileMap(1, B * H * W, cout, 0, _cus(ctx))
    gc.assert_turnover(tm)
    assert tm.NTL == 1 and tm.BN == 128
    x, w, b, slope, ref, _ = _conv_operands(ctx, "A", B, H, W, cin, cout, ("conv_turnover", "A"))
    got = _conv(ctx, x, w, b, slope, h2)
    _assert_exact(got, ref, tm, "A conv1x1 turn-over %s B=%d" % (NT_IDS[2 if h2 == "1" else 3], B))


@pytest.mark.parametrize("cout,cin,half", [c for c in CONV_SHAPES if c[0] in (85, 512)])
@pytest.mark.parametrize("h2", ["1", "0"], ids=["f16x2", "bf16x3"])
def test_conv1x1_heavy_tails(ctx, monkeypatch, cout, cin, half, h2):
    """family D with a random bias and slope 0.1, at the project's absolute bars relative to sum |x||w| + |b|"""
    _conv_env(monkeypatch, h2, half)
    B, H, W = 3, 13, 13
    x, w, b, slope, ref, scale = _conv_operands(ctx, "D", B, H, W, cin, cout, ("conv", cout, cin, "D"))
    got = _conv(ctx, x, w, b, slope, h2)
    _assert_bars(got, ref, scale, "conv1x1 %s Cin=%d Cout=%d DT_S3_HALF=%s" % (NT_IDS[2 if h2 == "1" else 3], cin, cout, half))
