"""The float64 reference of the Winograd transforms (tests/wino_transform_ref.py) against itself, without a GPU:
  - input transform, Winograd-domain product and output transform together are the direct 3x3 'same' convolution (all three tile sizes; with
    and without a mosaic, a ragged last group, pooled and not);
  - on the data of EVERY case of tests/test_gpu_wino_transform.py the conditions hold that make `array_equal` the right comparison there: the
    float32 evaluation in two different orders of summation equals the float64 one, and every expected value is a float32 number;
  - the split layouts round-trip bit for bit."""
import numpy as np
import pytest

import wino_transform_cases as wc
import wino_transform_ref as wr

REV = {ts: list(range(ts + 2))[::-1] for ts in (2, 4, 6)}


def _is_f32(a):
    return np.array_equal(np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64), np.asarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ the reference is a convolution
@pytest.mark.parametrize("ts", [2, 4, 6])
@pytest.mark.parametrize("B,H,W,pooled,mosaic", [(1, 7, 5, False, 0), (11, 13, 13, False, 0), (11, 13, 13, False, 1), (9, 5, 7, False, 0),
                                                 (5, 8, 14, True, 0), (11, 13, 13, True, 0), (2, 7, 5, False, 3), (37, 4, 4, True, 0)])
def test_transforms_are_the_direct_convolution(ts, B, H, W, pooled, mosaic):
    rs = np.random.RandomState(ts * 1000 + B * 10 + H)
    Cin, Cout = 3, 5
    x, w, b = rs.randn(B, H, W, Cin), rs.randn(3, 3, Cin, Cout), rs.randn(Cout)
    geo = wr.geometry(ts, B, H, W, pooled, mosaic)
    v = wr.input_transform(x, ts, geo)
    assert np.allclose(v, wr.input_transform(x, ts, geo, np.float64, REV[ts]), rtol=0, atol=1e-11)      # the two ways the reference evaluates Bt d B
    m = np.einsum("ptc,pnc->ptn", v, wr.filter_transform(w, ts))
    got = wr.output_transform(m, ts, geo, B, H, W, bias=b, slope=0.1)
    assert np.allclose(got, wr.output_transform(m, ts, geo, B, H, W, bias=b, slope=0.1, order=REV[ts]), rtol=0, atol=1e-11)
    want = wr.leaky(wr.conv_same(x, w) + b, 0.1)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max()) * (40 if ts == 6 else 4), (ts, np.abs(got - want).max())
    if pooled:
        p = wr.pool2(got)
        assert p.shape == (B, H // 2, W // 2, Cout)
        for i in range(H // 2):
            for j in range(W // 2):
                assert np.array_equal(p[:, i, j], got[:, 2 * i:2 * i + 2, 2 * j:2 * j + 2].max(axis=(1, 2)))


def test_geometry_rule_known_values():
    """the figures of the library's comment on its rule (network.hip: wino_geometry)"""
    assert wr.geometry(6, 16, 13, 13)["g"] == 3 and wr.geometry(6, 16, 13, 13)["th"] == 7
    assert wr.geometry(6, 16, 26, 26)["g"] == 2 and wr.geometry(6, 16, 26, 26)["th"] == 9
    assert wr.geometry(4, 16, 13, 13)["g"] == 2 and wr.geometry(4, 16, 13, 13)["th"] == 7
    g = wr.geometry(6, 16, 26, 26, pooled=True)
    assert (g["g"], g["ph"], g["th"]) == (3, 28, 14)
    g = wr.geometry(6, 48, 52, 52)
    assert (g["g"], g["ph"], g["th"]) == (6, 53, 53)
    assert wr.geometry(6, 48, 52, 52, pooled=True)["g"] == 1
    assert wr.geometry(6, 8, 13, 13)["g"] == 2 and wr.geometry(6, 3, 13, 13)["g"] == 1      # a batch fills the mosaic it takes
    g = wr.geometry(4, 11, 13, 13)
    assert (g["g"], g["Mt"], g["Mp"]) == (2, 147, 256)
    assert wr.geometry(4, 11, 13, 13, mosaic=1)["Mt"] == 11 * 16


def test_border_case_and_pool():
    k = wr.border_case(1, 1)
    assert k.tolist() == [[15]]
    k = wr.border_case(3, 4)
    assert k[0, 0] == 5 and k[0, 3] == 9 and k[2, 0] == 6 and k[2, 3] == 10 and k[1, 1] == 0 and k[1, 0] == 4 and k[0, 1] == 1
    y = np.arange(2 * 5 * 3 * 1, dtype=np.float64).reshape(2, 5, 3, 1)
    assert wr.pool2(y).shape == (2, 2, 1, 1) and wr.pool2(y)[1, 1, 0, 0] == y[1, 3, 1, 0]


# ------------------------------------------------------------------------------------------------ exactness conditions of the GPU cases
def _thin(k):
    """the big cases: every 16th channel of the case's data (the condition is a property of the values, not of how many there are)"""
    return 16 if k["big"] else 1


@pytest.mark.parametrize("name", list(wc.INPUT_CASES))
def test_input_case_is_exact_in_float32(name):
    k = wc.INPUT_CASES[name]
    x = wc.input_data(name)[..., ::_thin(k)]
    assert x.min() >= -128 and x.max() <= 127 and np.array_equal(x, np.round(x))
    ts = k["ts"]
    geo = wr.geometry(ts, k["B"], k["H"], k["W"], k["pooled"], k["mosaic"])
    if k["mt_mod4"]:
        assert geo["Mt"] % 4 == k["mt_mod4"]
    v = wr.input_transform(x, ts, geo)
    assert _is_f32(v)
    assert np.array_equal(wr.input_transform(x, ts, geo, np.float32).astype(np.float64), v)
    assert np.array_equal(wr.input_transform(x, ts, geo, np.float32, REV[ts]).astype(np.float64), v)
    v32 = v.astype(np.float32)
    if k["nt"] == 3:      # three bf16 terms hold any float32
        words = wr.pack_bf16x3(v32, geo["Mp"], wc.SENTINEL16)
        assert np.array_equal(wr.unpack_bf16x3(words, geo["Mt"]), v)
        assert np.all(words[:, :, :, geo["Mt"]:] == wc.SENTINEL16)
    if k["nt"] == 2:      # two fp16 terms of the scaled V hold 22 bits: enough for these integers, so the terms' sum is V again
        am = np.abs(x).max()
        words = wr.pack_f16x2(v32, ts, am, geo["Mp"], wc.SENTINEL16)
        assert np.array_equal(wr.unpack_f16x2(words, ts, am, geo["Mt"]), v)
        xs = np.abs(v) * wr.h2_scale(ts, am)[:, None, None]
        assert xs.max() < 2.0 ** 15 and np.isfinite(words.view(np.float16)[:, :, :, :geo["Mt"]]).all()


@pytest.mark.parametrize("name", list(wc.OUTPUT_CASES))
def test_output_case_is_exact_in_float32(name):
    k = wc.OUTPUT_CASES[name]
    saved = wc.output_data

    def thin(n):
        geo, m, bias, bias16 = saved(n)
        s = _thin(k)
        return geo, m[..., ::s], None if bias is None else bias[::s], None if bias16 is None else bias16[:, ::s]
    try:
        wc.output_data = thin
        full, pooled, am = wc.output_expected(name)
        for dtype, order in ((np.float32, None), (np.float32, REV[k["ts"]])):
            f2, p2, a2 = wc.output_expected(name, dtype, order)
            for a, b in ((full, f2), (pooled, p2)):
                assert (a is None) == (b is None) and (a is None or (b.dtype == np.float32 and np.array_equal(b.astype(np.float64), a)))
            assert a2 == am
    finally:
        wc.output_data = saved
    assert (full is None) == (k["pool"] == 1) and (pooled is None) == (k["pool"] == 0)
    for a in (full, pooled):
        assert a is None or _is_f32(a)
    geo, m, bias, bias16 = saved(name)
    assert np.abs(m).max() <= wc.M_MAX[k["ts"]] and np.array_equal(m, np.round(m))
    assert k["slope"] in (1.0, 0.5, 0.25) and (not k["bias16"] or (k["slope"] == 1.0 and k["pool"] == 0))
    assert float(am) == np.abs(pooled if k["pool"] else full).max()


def test_at_f6_is_not_exact_beyond_its_range():
    """why |m| <= 3 for F(6x6): with |m| <= 7 the 10 fractional bits and 15 integer bits of At m A no longer fit a float32"""
    rs = np.random.RandomState(3)
    m = rs.randint(-7, 8, size=(64, 20000, 1)).astype(np.float32)
    y = wr.tile_outputs(m, 6)
    assert not np.array_equal(wr.tile_outputs(m, 6, np.float32).astype(np.float64), y)
    m = np.clip(m, -3, 3)
    assert np.array_equal(wr.tile_outputs(m, 6, np.float32, REV[6]).astype(np.float64), wr.tile_outputs(m, 6))


# ------------------------------------------------------------------------------------------------ split layouts
@pytest.mark.parametrize("ts", [4, 6])
def test_split_layouts_round_trip_any_float32(ts):
    rs = np.random.RandomState(ts)
    P, Mt, C, Mp = (ts + 2) ** 2, 7, 48, 256
    v = (rs.randn(P, Mt, C) * np.exp(rs.randn(P, Mt, C) * 3)).astype(np.float32)
    words = wr.pack_bf16x3(v, Mp, wc.SENTINEL16)
    assert words.shape == (P, 3, C // 16, Mp, 16) and words.dtype == np.uint16
    assert np.array_equal(wr.unpack_bf16x3(words, Mt).astype(np.float32).view(np.uint32), v.view(np.uint32))
    # element (p, tile, c) lies at [p][term][c / 16][tile][c % 16]
    assert words[5, 0, 2, 3, 7] == wr.bf16_round(v[5, 3, 39]) and np.all(words[:, :, :, Mt:] == wc.SENTINEL16)
    # fp16 form: integers below 2^19 in magnitude relative to a 2^7 maximum survive the two terms
    vi = rs.randint(-15000, 15001, size=(P, Mt, C)).astype(np.float32)
    words = wr.pack_f16x2(vi, ts, 100.0, Mp, wc.SENTINEL16)
    assert words.shape == (P, 2, C // 16, Mp, 16)
    assert np.array_equal(wr.unpack_f16x2(words, ts, 100.0, Mt), vi.astype(np.float64))
    s = wr.h2_scale(ts, 100.0)
    assert s[0] == 2.0 ** (14 - 6) / 256 and s[3 * (ts + 2) + 4] == 2.0 ** 8 / 64 and wr.h2_scale(ts, 128.0)[0] == 2.0 ** 7 / 256
    hi = (vi[5, 3, 39] * np.float32(s[5])).astype(np.float16)
    assert words[5, 0, 2, 3, 7] == hi.view(np.uint16)


def test_bf16_round_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0], dtype=np.float32)
    assert wr.bf16_value(wr.bf16_round(x)).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0]


# ------------------------------------------------------------------------------------------------ the gate cases
@pytest.mark.parametrize("name", list(wc.GATE_CASES))
def test_gate_case_design_and_tolerance_baseline(name):
    k = wc.GATE_CASES[name]
    geo, m, xproj, c, z = wc.gate_data(name)
    ts, B, H, W, U = k["ts"], k["B"], k["H"], k["W"], k["U"]
    # z is exact: At m A in float32 (two orders) is the float64 one, xproj and c are float32 numbers, and float32(y + xproj) is the designed z
    y = wr.frames_from_tiles(wr.tile_outputs(m, ts), ts, geo, B, H, W)
    for order in (None, REV[ts]):
        y32 = wr.frames_from_tiles(wr.tile_outputs(m, ts, np.float32, order), ts, geo, B, H, W)
        assert y32.dtype == np.float32 and np.array_equal(y32.astype(np.float64), y)
    assert _is_f32(xproj) and _is_f32(c)
    assert np.array_equal((y32 + xproj.astype(np.float32)).astype(np.float64), z)
    c64, h64 = wr.gate_update(z, c)
    c32, h32 = wr.gate_update(z, c, np.float32)
    dc, dh = np.abs(c32 - c64).max(), np.abs(h32 - h64).max()
    print("gate tolerance baseline %s: |c32 - c64| %.3g  |h32 - h64| %.3g" % (name, dc, dh))
    if k["mode"] == "sat":
        col = wr.gate_columns(U)
        for g in (0, 1, 3):
            assert set(np.unique(wr.hard_sigmoid(z[..., col[g]].astype(np.float32)))) == {0.0, 0.5, 1.0}
        assert set(np.unique(np.tanh(z[..., col[2]].astype(np.float32)))) == {-1.0, 1.0}
        assert dc == 0 and _is_f32(c64)                  # c_out: bit for bit
        assert 4 * dh <= wc.GATE_H_TOL_SAT
    else:
        assert 4 * dh <= wc.GATE_H_TOL_SOFT and 4 * dc <= wc.GATE_C_TOL_SOFT
        assert len(np.unique(wr.hard_sigmoid(z))) > 20


def test_gate_tolerances_are_four_baselines():
    """the constants are 4 x the LARGEST baseline over their cases, not more"""
    worst = {"sat": 0.0, "soft_h": 0.0, "soft_c": 0.0}
    for name, k in wc.GATE_CASES.items():
        _, _, _, c, z = wc.gate_data(name)
        c64, h64 = wr.gate_update(z, c)
        c32, h32 = wr.gate_update(z, c, np.float32)
        if k["mode"] == "sat":
            worst["sat"] = max(worst["sat"], np.abs(h32 - h64).max())
        else:
            worst["soft_h"] = max(worst["soft_h"], np.abs(h32 - h64).max())
            worst["soft_c"] = max(worst["soft_c"], np.abs(c32 - c64).max())
    for tol, key in ((wc.GATE_H_TOL_SAT, "sat"), (wc.GATE_H_TOL_SOFT, "soft_h"), (wc.GATE_C_TOL_SOFT, "soft_c")):
        assert 4 * worst[key] <= tol <= 4.04 * worst[key], (key, worst[key])      # (the constants are written with three digits)


def test_gate_columns_layout():
    col = wr.gate_columns(96)
    assert col[0, 0] == 0 and col[1, 0] == 32 and col[3, 31] == 127 and col[0, 32] == 128 and col[2, 95] == 256 + 64 + 31
    assert sorted(col.reshape(-1).tolist()) == list(range(384))
