"""CPU suite: the claims tests/test_gpu_conv_igemm_edges.py rests on, proven on the numpy model of tests/conv_igemm_cases.py.

  * the restated tile schedule visits every tile exactly once -- for every case of the table and exhaustively at small sizes;
  * every family-A (and As, H) case keeps its sums below 2^24, so "bit for bit" is a fair demand of a float32 kernel;
  * the references equal the oracle's conv2d / maxpool2 / space_to_depth2 / convlstm_step to their float32 rounding;
  * the model, which computes tiles as scheduled, equals the direct convolution -- and stops doing so under each defect a case claims to see;
  * the table reaches all 35 instances launch_conv_igemm can dispatch."""
import numpy as np
import pytest

import conv_igemm_cases as cc


def _tiles(k):
    e = cc.expected_info(k)
    return e["BM"], e["BN"], e["grid_x"]


def _schedule(k):
    BM, BN, G = _tiles(k)
    M = k["W"] if k["P"] > 1 else k["B"] * k["H"] * k["W"]
    return cc.Schedule(M, k["N"], BM, BN, k["P"], cc.tile_gn_of(k["ks"], k["kind"]), G)


def test_tile_map_is_a_bijection_for_every_case():
    for k in cc.CASES.values():
        assert _schedule(k).is_bijection(), k["name"]


def test_tile_map_is_a_bijection_exhaustively_at_small_sizes():
    for ntn in range(1, 7):
        for gn in (0, 1, 2, 3):
            for total in range(ntn, 301, ntn):
                ntm = total // ntn
                tiles = {cc.tile_of(L, total, ntm, ntn, gn) for L in range(total)}
                assert len(tiles) == total and all(z == 0 and 0 <= tm < ntm and 0 <= tn < ntn for z, tm, tn in tiles), (total, ntn, gn)
    # the walk L = b, b + G, ... covers [0, total) once for any G; with the map above a bijection, so does the schedule (spot-checked whole)
    for total in (1, 7, 8, 12, 59, 300):
        for G in range(1, 41):
            assert sorted(L for b in range(min(G, total)) for L in range(b, total, G)) == list(range(total))
    for total, G, ntn, gn in ((12, 5, 2, 2), (300, 40, 6, 2), (295, 37, 5, 2), (21, 8, 3, 2), (6, 4, 2, 2)):
        assert cc.bijective(total, G, ntn, gn)


def test_batched_problems_share_one_tile_index():
    s = cc.Schedule(130, 256, 128, 128, 3, 2, 5)
    assert s.total == 12 and s.is_bijection() and s.max_turns() == 3
    assert {z for z, _, _ in s.tiles} == {0, 1, 2}
    # q = 1, r = 4: XCDs 0..3 own two consecutive tile numbers, 4..7 one
    assert [s.tiles[L] for L in (0, 8)] == [cc.tile_of(0, 12, 2, 2, 2), cc.tile_of(8, 12, 2, 2, 2)]
    d = s.locate(2, 129, 255)
    assert s.tiles[d["L"]] == (2, 1, 1) and d["workgroup"] == d["L"] % 5 and d["turn"] == d["L"] // 5


def test_narrow_last_column_group():
    # three column tiles in groups of two: the last group is one tile wide and walks the row tiles one by one
    order = [cc.tile_of(L, 6, 2, 3, 2)[1:] for L in range(6)]
    assert sorted(order) == [(m, n) for m in range(2) for n in range(3)]
    assert {cc.tile_of(L, 6, 2, 3, 2, gw_is_gn=True)[1:] for L in range(6)} != set(order)


def test_split_ranges_and_k_order():
    assert cc.split_ranges(9, 2) == [(0, 4), (4, 5)]                       # starts mid-way through the nine taps
    assert cc.split_ranges(9, 9) == [(i, 1) for i in range(9)]             # one chunk per split
    assert cc.split_ranges(18, 5) == [(0, 3), (3, 4), (7, 3), (10, 4), (14, 4)]      # [7, 10) crosses the 32-channel slice at chunk 9
    for nk, S in ((9, 4), (36, 6), (3, 2), (12, 2)):
        r = cc.split_ranges(nk, S)
        assert r[0][0] == 0 and sum(n for _, n in r) == nk and all(n >= 1 for _, n in r)
        assert all(r[i][0] + r[i][1] == r[i + 1][0] for i in range(S - 1))
    assert cc.k_index(0, 1, 9) == 32 and cc.k_index(32, 0, 9) == 9 * 32 and cc.k_index(33, 8, 9) == (9 + 8) * 32 + 1


def test_exact_families_stay_below_2_24():
    for k in cc.CASES.values():
        if k["fam"] == "D":
            continue
        o = cc.operands(k)
        K = k["ks"] ** 2 * k["Cin"]
        bound = K * float(np.abs(o["x"]).max()) * float(np.abs(o["w"]).max()) + 16      # any partial sum of any order, + bias / xproj
        assert bound < 2 ** 24, (k["name"], bound)
        for a in o.values():
            assert a is None or (np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 8), k["name"]


def test_family_d_has_no_denormals_and_spans_13_binades():
    o = cc.operands(cc.CASES["K_3x3_Cin64_D"])
    for a in (o["x"], o["w"]):
        assert np.all(np.abs(a[a != 0]) > 2.0 ** -100)
    assert cc.d_bar(32, 1) < 2.0 ** -17 < 2.0 ** -11      # a dropped low half or a 10-bit mantissa errs by 2^-11


def test_references_match_the_oracle():
    from oracle import oracle as orc
    rs = np.random.RandomState(5)
    x = rs.randn(2, 6, 10, 32).astype(np.float32)
    for ks in (3, 1):
        w = (rs.randn(ks, ks, 32, 40) / np.sqrt(ks * ks * 32)).astype(np.float32)
        b = rs.randn(40).astype(np.float32)
        ref = cc.conv_same(x, w) + b.astype(np.float64)
        got = orc.conv2d(x, w, b)
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
        v = ref.astype(np.float32)
        assert np.array_equal(orc.maxpool2(v), cc.maxpool2(v))
        assert np.array_equal(orc.space_to_depth2(v), cc.space_to_depth2(v))
    U = 32
    h, c = rs.randn(2, 6, 10, U).astype(np.float32), rs.randn(2, 6, 10, U).astype(np.float32)
    Wk = (rs.randn(3, 3, 32, 4 * U) / 17).astype(np.float32)
    Uk = (rs.randn(3, 3, U, 4 * U) / 17).astype(np.float32)
    bias = rs.randn(4 * U).astype(np.float32)
    ho, co = orc.convlstm_step(x, h, c, Wk, Uk, bias)
    z = cc.conv_same(x, Wk) + cc.conv_same(h, Uk) + bias.astype(np.float64)
    # (hard_sigmoid32 is the kernel's single-rounding form for INTEGER z; on these reals it is within one float32 rounding of the oracle's)
    c_ref, h_ref = cc.gate_update(z, c)
    assert np.allclose(co, c_ref, rtol=cc.GATE_RTOL, atol=cc.GATE_ATOL) and np.allclose(ho, h_ref, rtol=cc.GATE_RTOL, atol=cc.GATE_ATOL)


def test_quad_row_order_and_gate_columns():
    b, h, w = cc.quad_rows(2, 4, 6)
    assert (b[4], h[4], w[4]) == (0, 0, 2) and (b[7], h[7], w[7]) == (0, 1, 3) and (b[24], h[24], w[24]) == (1, 0, 0)
    assert sorted(zip(b, h, w)) == sorted(zip(*cc.linear_rows(2, 4, 6)))
    n_map = cc.gate_columns(64)
    assert sorted(n_map) == list(range(256))
    assert n_map[0] == 0 and n_map[32] == 64 and n_map[96] == 192 and n_map[128] == 32 and n_map[128 + 32 + 5] == 64 + 32 + 5
    v = np.arange(2 * 4 * 6 * 3, dtype=np.float32).reshape(2, 4, 6, 3)
    s = cc.space_to_depth2(v)
    assert np.array_equal(s[1, 1, 2, 2 * 3:3 * 3], v[1, 3, 4]) and np.array_equal(s[0, 0, 0, 3:6], v[0, 0, 1])


def test_hard_sigmoid_is_rounded_once():
    z = np.arange(-4, 5)
    want = np.clip(np.array([np.float32(np.float64(np.float32(0.2)) * v + 0.5) for v in z]), 0, 1)
    assert np.array_equal(cc.hard_sigmoid32(z), want) and cc.hard_sigmoid32(np.array([0]))[0] == 0.5


def _equal_where_computed(Z, ref):
    return (not np.isnan(Z).any()) and np.array_equal(Z, ref.astype(np.float64))


MODEL_CASES = [k["name"] for k in cc.CASES.values() if k["pins"] or k["group"] in ("K", "S", "SK") or k["name"].startswith(("Q_pool_3x3_128x128", "Q_s2d_1x1_256x128"))]


@pytest.mark.parametrize("name", [n for n in MODEL_CASES if cc.CASES[n]["fam"] != "D"])
def test_model_as_scheduled_equals_the_direct_convolution(name):
    k = cc.CASES[name]
    o = cc.operands(k)
    BM, BN, G = _tiles(k)
    assert _equal_where_computed(cc.model_preact(k, o, BM, BN, G), cc.preact(k, o)), name


PIN_DEFECT = {"korder": "tap_outer", "split": "split_shift", "gw": "gw_is_gn", "turns": "stale_rows"}


@pytest.mark.parametrize("name,pin", [(k["name"], p) for k in cc.CASES.values() for p in k["pins"]])
def test_each_structural_claim_is_sensitive(name, pin):
    k = cc.CASES[name]
    o = cc.operands(k)
    BM, BN, G = _tiles(k)
    if pin == "turns":
        assert _schedule(k).max_turns() >= 2, name
    assert not _equal_where_computed(cc.model_preact(k, o, BM, BN, G, mutate=PIN_DEFECT[pin]), cc.preact(k, o)), (name, pin)


def test_every_defect_is_claimed_by_some_case():
    claimed = {p for k in cc.CASES.values() for p in k["pins"]}
    assert claimed == set(PIN_DEFECT)
    assert cc.CASES["P1_K32"]["Cin"] == 32      # nk == 1: the persistent kernel's inner chunk loop never runs
    s = _schedule(cc.CASES["P1_K32"])
    assert s.total == 7 and [len(range(b, 7, 3)) for b in range(3)] == [3, 2, 2]


def test_the_table_reaches_all_35_instances():
    reached = {cc.instance_of(k) for k in cc.CASES.values()}
    assert sorted(reached) == cc.ALL_INSTANCES
    # ... and the fallbacks are stated, not computed: 257 columns on 384 weight rows, the gate instances at U = 32 / 96
    assert cc.CASES["C_3x3_256x256_N257_npad384"]["runs"] == "256x128" and cc.CASES["G_3x3_256_U96_M130"]["runs"] == "128x128"
    assert cc.expected_info(cc.CASES["C_1x1_256x256_N257"])["BN"] == 256


def test_cases_are_small_and_aligned():
    for k in cc.CASES.values():
        assert k["Cin"] % 32 == 0 and k["in_ld"] % 4 == 0 and k["in_gap"] % 4 == 0 and k["col_off"] % 4 == 0, k["name"]
        cols = 4 * k["N"] if k["kind"] == "s2d" else (k["N"] // 4 if k["kind"] == "gates" else k["N"])
        assert (cols + k["out_extra"]) % 4 == 0, k["name"]
        assert k["kind"] != "pool_both" or (k["N"] + k["out2_extra"]) % 4 == 0, k["name"]
        assert k["kind"] != "gates" or ((k["N"] + k["xp_extra"]) % 4 == 0 and (cols + k["c_extra"]) % 4 == 0), k["name"]
        M = k["W"] if k["P"] > 1 else k["B"] * k["H"] * k["W"]
        assert max(k["P"], 1) * M * max(k["N"], k["Cin"]) <= 36 * 130 * 256, k["name"]
