"""CPU suite: the claims tests/test_gpu_conv1_edges.py rests on, proven on the numpy restatement of tests/conv1_cases.py.

  * the restated launcher rule gives the tiles per workgroup production is known to walk, and a walk covers every tile of a row exactly once;
  * the references equal the oracle chain maxpool2(bn_leaky(conv2d(normalize_u8(.)))) to float32 rounding;
  * every exact-family case keeps its sums -- in any order, under any term split -- below 2^24, so "bit for bit" is a fair demand;
  * the emulated three-term split passes family T on the committed inputs, and stops doing so with any single partial product dropped;
  * the case table reaches all four kernel instances, every walk kind on each of them, every slope of a family on each instance that runs it."""
import numpy as np
import pytest

import conv1_cases as c1


def _ntx(k):
    return -(-(k["W"] // 2) // 8)


def test_the_rule_as_production_walks():
    assert c1.plan(2, 416, 416, "u8")["tpw"] == 1 and c1.plan(12, 416, 416, "u8")["tpw"] == 4 and c1.plan(1440, 416, 416, "u8")["tpw"] == 26
    assert c1.plan(*c1.RULE_SHAPE, dtype="u8") == dict(instance=c1.INSTANCE_CODE[c1.FULL], tpw=2, grid_x=2, grid_y=1, grid_z=1024, fills_amax=1)
    for B, H, W in c1.PRODUCTION_SHAPES:      # the detector-level conv_1 test never walks
        assert c1.plan(B, H, W, "u8")["tpw"] == 1 and c1.plan(B, H, W, "f32")["tpw"] == 1
    # the instance: float32 frames never fall back; uint8 frames need W % 4 == 0 and a 4-byte aligned address, whole tiles need multiples of 16
    assert [c1.plan(2, 32, 32, "u8", align=a)["instance"] for a in range(4)] == [1, 0, 0, 0]
    assert [c1.plan(2, 32, 32, "f32", align=a)["instance"] for a in range(4)] == [3, 3, 3, 3]
    assert [c1.plan(2, H, W, "u8")["instance"] for H, W in ((16, 16), (16, 20), (18, 16), (16, 18), (14, 22))] == [1, 2, 2, 0, 0]
    assert c1.plan(2, 16, 16, "u8", split=0)["instance"] == 0 and c1.plan(2, 16, 16, "f32", split=0)["fills_amax"] == 0
    for bad in (dict(H=3), dict(W=5), dict(B=0), dict(B=65536), dict(slope=-0.1), dict(tpw=27)):
        assert c1.plan(**dict(dict(B=2, H=4, W=4, dtype="u8"), **bad)) is None, bad
    assert c1.plan(65535, 2, 2, "u8")["grid_z"] == 65535


def test_a_walk_covers_its_row_once():
    for inst in c1.INSTANCES:
        for ntx in range(1, 30):
            for tpw in range(1, c1.C1_TPW + 1):
                ws = c1.walks(ntx, tpw, inst)
                assert [t["bx"] for w in ws for t in w["tiles"]] == list(range(ntx))
                for w in ws:
                    last = w["tiles"][-1]["bx"]
                    for t in w["tiles"]:      # a request stays inside the walk; each tile but the first two (mfma: the first) was requested two (one) tiles ahead
                        assert t["request"] is None or w["tiles"][0]["bx"] <= t["request"] <= last
                        if inst == c1.FULL:
                            assert t["request"] == min(t["bx"] + 2, last) and t["loop"] == ("tail" if t["bx"] == last and len(w["tiles"]) % 2 else "pair")
                        assert t["set"] == ("A" if inst == c1.MFMA else "AB"[t["pos"] % 2])
    w = c1.walks(7, 3, c1.FULL)
    assert [[(t["bx"], t["set"], t["loop"], t["request"]) for t in g["tiles"]] for g in w] == [
        [(0, "A", "pair", 2), (1, "B", "pair", 2), (2, "A", "tail", 2)], [(3, "A", "pair", 5), (4, "B", "pair", 5), (5, "A", "tail", 5)], [(6, "A", "tail", 6)]]
    assert w[2]["kinds"] == {"single", "short"} and w[0]["kinds"] == {"odd"}
    k = c1.CASES["W_full_u8_I_2x16x112_t3"]
    d = c1.locate(k, 1, 5, 51, 9)
    assert d["tile"] == (0, 6) and d["workgroup"] == (2, 0, 1) and d["position"] == 0 and d["loop"] == "tail" and d["wave"] == 2 and d["group"] == 1 and d["lane"] == 41


def test_references_match_the_oracle_chain():
    from oracle import oracle as orc
    for name in ("W_full_u8_D_2x16x112_t3", "E_u8_u8_D_2x34x52_t0", "E_u8_u8_I_2x14x20_t0", "R_full_u8_P_2x48x16_t0"):
        k = c1.CASES[name]
        o = c1.operands(k)
        ones, zeros = np.ones(32, np.float32), np.zeros(32, np.float32)
        var = ones - np.float32(orc.BN_EPS)
        conv = orc.conv2d(orc.normalize_u8(o["frames"]), o["w"].reshape(3, 3, 3, 32))
        want = orc.maxpool2(orc.bn_leaky(conv, ones, o["bias"], zeros, var, alpha=k["slope"]))
        x = o["frames"].astype(np.float64) / 255.0
        ref = c1.layer64(c1.preact(x, o["w"].astype(np.float64)), o["bias"], k["slope"])
        scale = c1.cc.maxpool2(c1.preact_abs(x, o["w"], o["bias"]))
        # the oracle: float32 x/255, a float32 convolution of 27 terms, a batch norm whose 1/sqrt(var + eps) is 1 to a rounding, LeakyReLU
        assert np.all(np.abs(want.astype(np.float64) - ref) <= 2.0 * (27 + 5) * 2.0 ** -24 * scale), name
        if k["fam"] in ("I", "P"):      # and the exact integer reference is that same layer (b / 255 in float64 against w = 255 q, rounded twice)
            assert np.all(np.abs(c1.expected_exact(k, o) - ref) <= 4 * 2.0 ** -24 * scale), name


def test_exact_families_stay_below_2_24():
    for k in c1.CASES.values():
        if k["fam"] not in ("P", "I", "Ib", "Tp"):
            continue
        o = c1.operands(k)
        if k["fam"] in ("I", "Ib"):
            assert np.all(o["x"] == np.rint(o["x"])) and np.all(o["wx"] == np.rint(o["wx"])) and np.all(o["bias"] == np.rint(o["bias"]))
            assert c1.sum_bound(k, o) < 2.0 ** 24, (k["name"], c1.sum_bound(k, o))
            if k["dtype"] == "u8":      # w / 255 is exact: one bf16 term
                assert np.array_equal((o["w"].astype(np.float64) / 255.0).astype(np.float32), o["wx"].astype(np.float32)) and np.abs(o["wx"]).max() <= 4
            else:                        # at most 16 significant bits: two bf16 terms, the third is zero
                for v in (o["frames"], o["w"]):
                    assert not c1.split3(v)[2].any()
        elif k["fam"] == "P":
            assert np.count_nonzero(o["wx"]) == 32 and set(np.unique(o["wx"])) == {-1.0, 0.0, 1.0}
            if k["dtype"] == "f32":
                codes = o["frames"].ravel()
                assert len(np.unique(codes)) == codes.size and codes.min() >= 1 and codes.max() < 2.0 ** 24 and np.all(codes == np.rint(codes))
        else:
            assert np.all(np.abs(np.frexp(o["wx"][o["wx"] != 0])[0]) == 0.5)      # powers of two
    k = c1.CASES["M_u8_u8_Ib_2x14x20_t0"]
    o = c1.operands(k)
    want = c1.expected_exact(k, o)
    assert want.min() > 0 and want.max() < o["bias"].min()      # a window of padding alone evaluates to the bias: it would win the maximum


T_CASES = [n for n, k in c1.CASES.items() if k["fam"] == "T" and k["inst"] != c1.MFMA]


@pytest.mark.parametrize("name", T_CASES)
def test_split_emulation_passes_family_T_and_no_dropped_product_does(name):
    k = c1.CASES[name]
    o = c1.operands(k)
    ref = c1.layer64(c1.preact(o["x"], o["wx"]), o["bias"], k["slope"])
    nz = ref != 0
    assert nz.mean() > 0.9
    order = c1.U8_ORDER if k["dtype"] == "u8" else c1.F32_ORDER

    def err(drop):
        got = c1.emulate_layer(o["frames"], o["w"], o["bias"], k["slope"], drop).astype(np.float64)
        return np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])

    kept = err(None).max()
    assert kept <= c1.t_bar() / 4, (name, kept * 2.0 ** 24)      # (measured: at most 1.5 x 2^-24 on float32 frames, 1.9 x 2^-24 on uint8 frames)
    for d in range(len(order)):
        e = err(d)
        assert e.max() >= 125 * 2.0 ** -24 > c1.t_bar() and np.mean(e > 4 * 2.0 ** -24) > 0.85, (name, order[d], e.max() * 2.0 ** 24, np.mean(e > 4 * 2.0 ** -24))


def test_split_emulation_is_exact_on_the_exact_families():
    for name in ("W_full_u8_I_2x16x112_t3", "W_u8_u8_I_2x14x108_t3", "W_f32_f32_I_2x16x112_t3", "W_f32_f32_P_2x16x112_t3", "W_full_u8_P_2x16x112_t3",
                 "M_f32_f32_Ib_2x14x20_t0"):
        k = c1.CASES[name]
        o = c1.operands(k)
        assert np.array_equal(c1.emulate_layer(o["frames"], o["w"], o["bias"], k["slope"]), c1.expected_exact(k, o)), name
    k = c1.CASES["W_f32_f32_I_2x16x112_t3"]      # ... and family I sees a dropped product too (x2 w2 is the smallest that is not zero)
    o = c1.operands(k)
    for d in (1, 3, 4, 5):
        assert not np.array_equal(c1.emulate_layer(o["frames"], o["w"], o["bias"], k["slope"], d), c1.expected_exact(k, o)), d


def test_family_D_bar_holds_on_the_emulation():
    for name in ("W_full_u8_D_2x16x112_t3", "W_f32_f32_D_2x16x112_t3"):
        k = c1.CASES[name]
        o = c1.operands(k)
        ref = c1.layer64(c1.preact(o["x"], o["wx"]), o["bias"], k["slope"])
        e = np.abs(c1.emulate_layer(o["frames"], o["w"], o["bias"], k["slope"]).astype(np.float64) - ref) / c1.cc.maxpool2(c1.preact_abs(o["x"], o["wx"], o["bias"]))
        assert e.max() <= c1.d_bar1() == 2.0 ** -18


def test_table_reaches_every_instance_walk_kind_and_slope():
    for k in c1.CASES.values():
        assert k["want"] == c1.plan(k["B"], k["H"], k["W"], k["dtype"], k["align"], k["split"], k["tpw"], k["slope"]) and c1.INSTANCES[k["want"]["instance"]] == k["inst"]
    assert {k["inst"] for k in c1.CASES.values()} == set(c1.INSTANCES)
    for inst in c1.INSTANCES:
        mine = [k for k in c1.CASES.values() if k["inst"] == inst]
        kinds = set()
        for k in mine:
            for w in c1.walks(_ntx(k), k["want"]["tpw"], inst):
                kinds |= w["kinds"]
                if "short" in w["kinds"] and len(w["tiles"]) > 1:
                    kinds.add("short walk of several tiles")
        assert kinds == set(c1.WALK_KINDS) | {"short walk of several tiles"}, (inst, kinds)
        fams = {k["fam"] for k in mine}
        assert {"I", "D", "T"} <= fams and ("P" in fams) and (inst == c1.FULL or any(k["fam"] == "P" and k["dtype"] == "f32" for k in mine) or inst == c1.U8), (inst, fams)
        for fam in ("P", "I"):
            assert {k["slope"] for k in mine if k["fam"] == fam} == set(c1._SLOPES[fam]), (inst, fam)
        assert any(k["publish"] for k in mine)
    # the shapes the work asks for
    W = {(k["inst"], _ntx(k), k["tpw"]) for k in c1.by_group("W")}
    assert W >= {(i, n, t) for i in c1.INSTANCES for n in c1.WALK_NTX for t in c1.WALK_TPW}
    assert {(k["inst"], k["tpw"]) for k in c1.by_group("Wb")} == {(i, t) for i in c1.INSTANCES for t in (13, 26)} and all(_ntx(k) == 26 for k in c1.by_group("Wb"))
    E = {(k["H"], k["W"], k["inst"]) for k in c1.by_group("E")}
    assert E >= {(H, Wd, i) for H in (2, 6, 14, 18, 34) for Wd in (4, 12, 20, 36, 52) for i in (c1.U8, c1.F32)}
    E2 = {(k["W"], k["dtype"], k["inst"]) for k in c1.by_group("E2")}
    assert E2 == {(Wd, "u8", c1.MFMA) for Wd in (2, 6, 18, 22, 34)} | {(Wd, "f32", c1.F32) for Wd in (2, 6, 18, 22, 34)}
    assert {(k["align"], k["inst"], k["want"]["fills_amax"]) for k in c1.by_group("A")} == {(0, c1.FULL, 1), (1, c1.MFMA, 0), (2, c1.MFMA, 0), (3, c1.MFMA, 0)}
    assert {k["H"] for k in c1.by_group("R")} == {32, 48}
    assert all(k["B"] == 2 for k in c1.by_group("W", "Wb", "R", "E", "E2", "A", "M"))
    L = c1.by_group("L")
    assert {(k["B"], k["H"], k["W"]) for k in L} == {c1.RULE_SHAPE} | set(c1.PRODUCTION_SHAPES) and all(k["tpw"] == 0 for k in L)
