"""What tests/test_gpu_gemm_split_edges.py rests on, shown without a GPU on the numpy model of the split GEMM's arithmetic
(tests/gemm_split_cases.py: model_gemm, built on tests/test_split_arith.py):

  * families A and B are EXACT under the model, in both operand forms, at every K of the case table (and at K = 1024);
  * with one partial product left out, each in turn, the GPU file's assertion for a family fails or not as DETECTS states -- in
    particular the three smallest products of the bf16 form are invisible to A and B (zero, or below the rounding) and it is D's bars
    that catch them;
  * the tile map the failure messages use visits every tile exactly once, for every case of the table."""
import numpy as np
import pytest

import gemm_split_cases as gc

K_VALUES = gc.table_k_values() + [1024]


def _small(family, K, seed):
    return gc.FAMILIES[family](2, 40, K, 48, seed)


def _exact(family, v, u):
    ref, _ = gc.reference(v, u)
    return ref.astype(np.float32)


def test_table_k_values_are_what_the_issue_lists():
    assert gc.table_k_values() == [32, 64, 96, 160]


@pytest.mark.parametrize("K", K_VALUES)
@pytest.mark.parametrize("nt", [2, 3], ids=["f16x2", "bf16x3"])
@pytest.mark.parametrize("family", ["A", "B"])
def test_families_a_and_b_are_exact_on_the_model(family, nt, K):
    v, u = _small(family, K, 100 + K)
    want = _exact(family, v, u)
    got = gc.model_gemm(v, u, nt)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    if family == "A":      # the integer product itself
        assert np.array_equal(want.astype(np.int64), np.einsum("pmk,pnk->pmn", v.astype(np.int64), u.astype(np.int64)))
        assert np.abs(want).max() < 2 ** 24


def test_family_operands_are_what_the_docstring_says():
    v, u = gc.family_a(2, 40, 96, 48, 1)
    assert np.array_equal(v, np.round(v)) and np.abs(v).max() == 8 and np.abs(u).max() == 8 and v.min() == -8
    for x in (v, u):      # first term alone, in both splits
        assert np.array_equal(gc.split3(x)[0], x) and np.array_equal(gc.split2(x * np.float32(2.0 ** 11))[0].astype(np.float32), x * 2.0 ** 11)
    v, u = gc.family_b(2, 40, 96, 48, 2)
    assert ((v != 0).sum(-1) <= 8).all() and ((v != 0).sum(-1) >= 1).all() and (u > 0).all() and (v >= 0).all()
    for x in (v, u):
        n = np.round(x)
        assert np.array_equal(x.astype(np.float64), n * (1.0 + gc.B_EPS)) and n.max() == 8
        t3, t2 = gc.split3(x), gc.split2(x * np.float32(2.0 ** 11))
        assert np.array_equal(t3[0], n) and np.array_equal(t3[1].astype(np.float64), n * gc.B_EPS) and not t3[2].any()
        assert np.array_equal(t2[0].astype(np.float64), n * 2.0 ** 11) and np.array_equal(t2[1].astype(np.float64), n * 0.25)
    v, u = gc.family_d(2, 40, 96, 48, 3)
    assert v.dtype == u.dtype == np.float32
    assert np.log2(np.abs(v).max() / np.median(np.abs(v))) > 7      # heavy tails: the largest value far above the typical one


# Which family's assertion in the GPU file FAILS when the kernel loses one partial product (everywhere): product name -> families.
# A sees only the leading product, B the leading and the two cross products of weight 2^-8 (bf16) / 2^-11 (fp16).  The bf16 form's
# three smallest products (weight 2^-16) are zero on A, and on B either zero (u3 = v3 = 0) or, u2 v2 = 2^-26 of the result, below a
# quarter of its last place: only D's absolute bars see them.
DETECTS = {
    (2, "uhi_vhi"): "ABD", (2, "uhi_vlo"): "BD", (2, "ulo_vhi"): "BD",
    (3, "u1v1"): "ABD", (3, "u1v2"): "BD", (3, "u2v1"): "BD",
    (3, "u1v3"): "D", (3, "u2v2"): "D", (3, "u3v1"): "D",
}


@pytest.mark.parametrize("K", [32, 160, 1024])
@pytest.mark.parametrize("nt,name", sorted(DETECTS))
def test_a_dropped_product_fails_the_gpu_assertions(nt, name, K):
    drop = gc.PRODUCT_NAMES[nt].index(name)
    for family in "AB":
        v, u = _small(family, K, 200 + K)
        want = _exact(family, v, u)
        got = gc.model_gemm(v, u, nt, drop=drop)
        wrong = got != want
        if family in DETECTS[(nt, name)]:
            assert wrong[want != 0].all() and (want != 0).mean() > 0.95, (family, name, int(wrong.sum()))      # every element moves: a part of a tile cannot hide
            ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            ulp = ulp[want != 0]
            # the cross products carry 2^-13 of the result each: 1024 places of float32's last; hi hi carries the result's leading bits
            assert ulp.min() >= (1024 if "lo" in name or "2" in name else 2 ** 22), (family, name, int(ulp.min()))
        else:
            assert not wrong.any(), (family, name, int(wrong.sum()))
    v, u = _small("D", K, 300 + K)
    ref, scale = gc.reference(v, u)
    rms0, max0 = gc.d_error(gc.model_gemm(v, u, nt), ref, scale)
    assert gc.d_passes(rms0, max0) and rms0 < 0.9 * 2.0 ** -24 and max0 < 8 * 2.0 ** -24, (rms0, max0)      # the intact kernel: far inside
    rms, mx = gc.d_error(gc.model_gemm(v, u, nt, drop=drop), ref, scale)
    print("K=%d %s without %s: family D rms %.2f max %.1f (x 2^-24; intact %.2f / %.1f)" % (K, "f16x2" if nt == 2 else "bf16x3", name, rms * 2 ** 24, mx * 2 ** 24, rms0 * 2 ** 24, max0 * 2 ** 24))
    assert not gc.d_passes(rms, mx), (name, rms * 2 ** 24, mx * 2 ** 24)
    assert rms > 2 * gc.D_RMS_BAR      # ... and by its rms bar alone, with a factor to spare


def test_a_dropped_product_in_the_bias_stage_shows_on_integers():
    """the 1x1 layers' bias: one extra K stage in the bf16 form (its leading term rides on u1v1), one fma in the fp16 form"""
    rs = np.random.RandomState(7)
    v, u = gc.family_a(1, 40, 32, 48, 7)
    bias = rs.randint(-100, 101, 48).astype(np.float32)
    ref = np.einsum("pmk,pnk->pmn", v.astype(np.float64), u.astype(np.float64)) + bias.astype(np.float64)
    want = np.where(ref > 0, ref, ref * 0.5).astype(np.float32)
    assert np.array_equal(np.where(ref > 0, ref, ref * 0.5), want.astype(np.float64))      # halves of integers: exact
    for nt in (2, 3):
        assert np.array_equal(gc.model_gemm(v, u, nt, bias=bias, slope=0.5), want)
    assert np.array_equal(gc.split3(bias)[0], bias)      # 7 bits: the first bf16 term alone
    lost = gc.model_gemm(v, u, 3, bias=bias, slope=0.5, drop=5) != want
    assert lost[want != 0].all() and (want != 0).mean() > 0.95


@pytest.mark.parametrize("cus", [256, 304, 100])
def test_tile_map_visits_every_tile_once(cus):
    for name, tm, turn in gc.all_tile_maps(cus):
        seen = np.zeros(tm.tiles, np.int64)
        for w in range(tm.G):
            seq = tm.sequence(w)
            np.add.at(seen, seq, 1)
            for turn_no in {0, len(seq) - 1}:
                L = seq[turn_no]
                p, r = divmod(L, tm.MT * tm.NTL)
                mt, nt = divmod(r, tm.NTL)
                assert tm.locate(p, mt * tm.BM, nt * tm.BN) == (L, w, turn_no), (name, w, L)
        assert (seen == 1).all(), (name, cus, np.flatnonzero(seen != 1)[:8])
        assert tm.G <= tm.tiles and tm.xcd_order == (tm.G % 8 == 0)
        if turn:
            gc.assert_turnover(tm)


def test_tile_map_at_256_cus_is_what_the_table_promises():
    tms = {name: tm for name, tm, _ in gc.all_tile_maps(256)}
    t = tms["wino:one_row_k32"]; assert (t.tiles, t.G, t.BN, t.BM) == (1, 1, 128, 256)
    assert [tms["wino:rows%d" % m].tiles for m in (255, 256, 257)] == [3, 3, 6] and not tms["wino:rows257"].xcd_order
    t = tms["wino:bn128_30tiles"]; assert (t.tiles, t.BN, t.xcd_order) == (30, 128, False)
    t = tms["wino:bn256_ragged"]; assert (t.tiles, t.BN, t.MT) == (18, 256, 3)
    for k in ("wino:turnover_k32", "wino:turnover_k96"):
        t = tms[k]; assert (t.tiles, t.G, t.BN, t.xcd_order, t.max_turns()) == (768, 256, 128, True, 3)
    t = tms["wino:half_turnover"]; assert (t.tiles, t.G, t.BM, t.BN, t.xcd_order, t.max_turns()) == (1280, 512, 128, 256, True, 3)
    t = tms["wino:half_step_shape"]; assert (t.tiles, t.G, t.BM) == (360, 360, 128)
    t = tms["wino:g14_identity"]; assert (t.tiles, t.G, t.BN, t.xcd_order) == (14, 14, 256, False)
    t = tms["rows:turnover_n384"]; assert (t.BN, t.NTL, t.G, t.half_form) == (128, 3, 256, False) and t.max_turns() == 3
    t = tms["rows:turnover_n512"]; assert (t.BN, t.NTL, t.G, t.half_form) == (256, 2, 256, False) and t.max_turns() == 3
    assert tms["conv:512_half1"].half_form and tms["conv:512_half1"].tiles == 8 and not tms["conv:512_half0"].half_form
    assert not tms["conv:384_half1"].half_form and tms["conv:85_half0"].NTL == 1 and tms["conv:200_half0"].NTL == 2
    t = tms["conv:turnover"]; assert (t.tiles, t.G, t.BN, t.max_turns()) == (640, 256, 128, 3)
    # a tile's turn: workgroup 0 of the XCD order starts at tile 0, workgroup 1 at G / 8
    assert tms["wino:turnover_k32"].locate(0, 0, 0) == (0, 0, 0) and tms["wino:turnover_k32"].locate(0, 0, 128) == (1, 8, 0)
    assert tms["wino:turnover_k32"].first(1) == 32 and tms["wino:turnover_k32"].locate(63, 768, 383) == (767, 255, 2)


def test_a_mismatch_is_reported_with_its_tile_workgroup_and_turn():
    """the GPU file's equality assertion on host tensors: one wrong element of a turn-over case names tile, workgroup and turn"""
    import torch
    from test_gpu_gemm_split_edges import _assert_exact
    P, Mt, N = 2, 769, 384
    tm = gc.TileMap(P, Mt, N, -1, 16)      # 2 x 4 x 3 = 24 tiles on 16 workgroups, XCD order
    ref = torch.arange(P * Mt * N, dtype=torch.float64).reshape(P, Mt, N) % 97.0
    got = ref.float()
    _assert_exact(got, ref, tm, "A intact")
    got[1, 300, 260] += 1.0      # plane 1, second row tile, third column tile: L = (1 * 4 + 1) * 3 + 2 = 17 -> workgroup 8's second tile
    got[1, 700, 5] = float("nan")
    with pytest.raises(pytest.fail.Exception) as info:
        _assert_exact(got, ref, tm, "A broken")
    msg = str(info.value)
    assert "2 of %d elements wrong" % (P * Mt * N) in msg and "(p, m, n) = (1, 300, 260)" in msg, msg
    assert "tile 17 of 24, workgroup 8 of 16, turn 1" in msg and tm.sequence(8) == [1, 17], msg
