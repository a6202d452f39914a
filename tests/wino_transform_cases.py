"""The cases of tests/test_gpu_wino_transform.py, with their data: shared with tests/test_wino_transform_cpu.py, which re-checks on every
case's own data the conditions that make `array_equal` the right comparison (exact in float32 in any order; the float64 result a float32).

Value ranges (Bt and At hold dyadic rationals only, so the transforms are exact on small integers):
  input  x   integers in -128..127                     |Bt d B| <= 15637 (F6), 10455 (F4)
  M'         integers, |m| <= 3 (F6), <= 100 (F4, F2)  |At m A| <= 13492 with 10 fractional bits (F6): below 2^14 WITH the biases
  bias       integers, |b| <= 50; bias16 |b| <= 20;  slopes 1, 0.5, 0.25 (powers of two: the product is exact)"""
import zlib

import numpy as np

import wino_transform_ref as wr

M_MAX = {6: 3, 4: 100, 2: 100}
BIAS_MAX, BIAS16_MAX = 50, 20
SENTINEL32 = 0xFFC5A5A5      # a NaN as float32: an owned word that was never written cannot compare equal
SENTINEL16 = 0x7E5A          # a NaN as fp16, 1.8e38 as bf16

# (B, H, W, pooled, DT_WINO_MOSAIC)
GEOS = {
    "one_7x5": (1, 7, 5, False, 0),              # one frame, ragged H and W
    "b11_13x13": (11, 13, 13, False, 0),         # g = 3 (F6) / 2 (F4), ragged last group
    "b9_5x7": (9, 5, 7, False, 0),               # not square
    "pool_8x14": (5, 8, 14, True, 0),            # the pooled (even) pitch
    "nomosaic_13x13": (11, 13, 13, False, 1),    # DT_WINO_MOSAIC=1
    "mosaic3_b2_7x5": (2, 7, 5, False, 3),       # DT_WINO_MOSAIC=3 on two frames: seven absent frames in the group
}
SMALL = {6: "coop6", 4: "tpi4", 2: "tpi2"}      # the fp32 input kernel of a small launch


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def _case(**kw):
    d = dict(ld=None, bs_extra=0, nt=0, force=0, cap=False, threads=None, big=False, mt_mod4=None)
    d.update(kw)
    return d


def _input_cases():
    c = {}
    for ts in (2, 4, 6):
        for gname, (B, H, W, pooled, mosaic) in GEOS.items():
            c["f32_F%d_%s" % (ts, gname)] = _case(ts=ts, B=B, H=H, W=W, C=8, pooled=pooled, mosaic=mosaic, form=SMALL[ts], threads=256 if ts == 6 else 64)
        B, H, W, pooled, mosaic = GEOS["b11_13x13"]
        wide = dict(ts=ts, B=B, H=H, W=W, C=12, ld=20, bs_extra=8, pooled=False, mosaic=0)      # in_ld > C, frames apart
        c["f32_F%d_ld20" % ts] = _case(form=SMALL[ts], threads=256 if ts == 6 else 64, **wide)
        c["f32_F%d_ld20_cap" % ts] = _case(form=SMALL[ts], cap=True, **wide)
    wide6 = dict(ts=6, B=11, H=13, W=13, C=12, ld=20, bs_extra=8, pooled=False, mosaic=0)
    c["f32_F6_forced_tpi6"] = _case(form="tpi6", force=1, threads=64, **wide6)
    c["f32_F6_forced_tpi6_cap"] = _case(form="tpi6", force=1, cap=True, **wide6)
    c["f32_F6_forced_tpi6_pool"] = _case(ts=6, B=5, H=8, W=14, C=8, pooled=True, mosaic=0, form="tpi6", force=1)
    c["f32_F6_forced_coop6"] = _case(form="coop6", force=2, **wide6)
    # the launchers' thresholds, from either side.  13x13, B = 11: Mt = 98 (F6, g = 3), 147 (F4, g = 2), 539 (F2)
    big = dict(B=11, H=13, W=13, pooled=False, mosaic=0)
    c["f32_F6_tpi6_at_196608_pairs"] = _case(ts=6, C=4016, form="tpi6", threads=256, big=True, **big)       # 98 * 2008 = 196784
    c["f32_F6_coop6_below_196608_pairs"] = _case(ts=6, C=4012, form="coop6", threads=256, big=True, **big)  # 98 * 2006 = 196588
    c["f32_F4_256_threads_at_131072"] = _case(ts=4, C=3568, form="tpi4", threads=256, big=True, **big)      # 147 * 892 = 131124
    c["f32_F4_64_threads_below_131072"] = _case(ts=4, C=3564, form="tpi4", threads=64, big=True, **big)     # 147 * 891 = 130977
    c["f32_F2_256_threads_at_131072"] = _case(ts=2, C=976, form="tpi2", threads=256, big=True, **big)       # 539 * 244 = 131516
    c["f32_F2_64_threads_below_131072"] = _case(ts=2, C=972, form="tpi2", threads=64, big=True, **big)      # 539 * 243 = 130977
    # the split producers: Mt % 4 = 1, 2, 3 (their items are groups of four tiles), C = 32 (one K-block pair) and 96 (three)
    split_geos = {6: [(1, 13, 13), (11, 13, 13), (3, 6, 5)], 4: [(5, 4, 4), (1, 5, 9), (11, 13, 13)]}
    for form, ts, nt in (("s3_6", 6, 3), ("h2_6", 6, 2), ("s3_4", 4, 3), ("h2_4", 4, 2)):
        for i, (B, H, W) in enumerate(split_geos[ts]):
            c["%s_mt%d_c32" % (form, i + 1)] = _case(ts=ts, B=B, H=H, W=W, C=32, pooled=False, mosaic=0, nt=nt, form=form, threads=128, mt_mod4=i + 1)
        c["%s_c96_ld100" % form] = _case(ts=ts, B=11, H=13, W=13, C=96, ld=100, pooled=False, mosaic=0, nt=nt, form=form, threads=128)
        c["%s_c96_cap" % form] = _case(ts=ts, B=11, H=13, W=13, C=96, pooled=False, mosaic=0, nt=nt, form=form, cap=True)
        c["%s_c64_pool_8x14" % form] = _case(ts=ts, B=5, H=8, W=14, C=64, pooled=True, mosaic=0, nt=nt, form=form)
    # C % 16 == 0, C % 32 != 0: F(4x4) only, one thread per (tile, 4 channels)
    c["tpi4_s3_c48"] = _case(ts=4, B=11, H=13, W=13, C=48, pooled=False, mosaic=0, nt=3, form="tpi4_s3", threads=64)
    c["tpi4_s3_c48_cap"] = _case(ts=4, B=11, H=13, W=13, C=48, pooled=False, mosaic=0, nt=3, form="tpi4_s3", cap=True)
    c["tpi4_s3_c16_one_7x5"] = _case(ts=4, B=1, H=7, W=5, C=16, ld=24, pooled=False, mosaic=0, nt=3, form="tpi4_s3", threads=64)
    return c


INPUT_CASES = _input_cases()


def input_data(name):
    """x [B, H, W, C] float32, integers in -128..127 (both ends present)"""
    k = INPUT_CASES[name]
    rs = np.random.RandomState(_seed(name))
    x = rs.randint(-128, 128, size=(k["B"], k["H"], k["W"], k["C"])).astype(np.float32)
    x.reshape(-1)[rs.randint(x.size)] = -128.0
    return x


OUT_SMALL = {6: "coop6", 4: "tpi4", 2: "tpi2"}


def _ocase(**kw):
    d = dict(N=8, m_ld=None, out_ld=None, out2_ld=None, pool=0, slope=1.0, bias=True, bias16=False, mosaic=0, force=0, cap=False, threads=None, big=False)
    d.update(kw)
    return d


def _output_cases():
    c = {}
    slopes = (1.0, 0.5, 0.25)
    for ts in (2, 4, 6):
        forms = [(0, OUT_SMALL[ts], "")] + ([(1, "tpi6", "_tpi6")] if ts == 6 else [])
        for force, form, tag in forms:
            n = 0
            for gname, (B, H, W, pooled, mosaic) in GEOS.items():
                if pooled:
                    continue
                c["F%d%s_%s" % (ts, tag, gname)] = _ocase(ts=ts, B=B, H=H, W=W, slope=slopes[n % 3], mosaic=mosaic, force=force, form=form, bias=n != 1)
                n += 1
            for pool in (1, 2):
                c["F%d%s_pool%d_8x14" % (ts, tag, pool)] = _ocase(ts=ts, B=5, H=8, W=14, pool=pool, slope=slopes[pool], force=force, form=form)
            # odd H, W with pooling: MaxPooling2D drops the last row and column; 13x13 in a mosaic at the even pitch 14
            c["F%d%s_pool2_odd_7x5" % (ts, tag)] = _ocase(ts=ts, B=3, H=7, W=5, pool=2, slope=0.5, force=force, form=form)
            c["F%d%s_pool1_odd_b11_13x13" % (ts, tag)] = _ocase(ts=ts, B=11, H=13, W=13, pool=1, slope=0.25, force=force, form=form)
            wide = dict(ts=ts, B=11, H=13, W=13, N=8, m_ld=12, out_ld=20, out2_ld=12, pool=2, slope=0.5, force=force, form=form)      # out_ld > N
            c["F%d%s_ld20" % (ts, tag)] = _ocase(threads=256 if form == "coop6" else 64, **wide)
            c["F%d%s_ld20_cap" % (ts, tag)] = _ocase(cap=True, **wide)
            c["F%d%s_full_cap" % (ts, tag)] = _ocase(ts=ts, B=11, H=13, W=13, N=8, out_ld=12, cap=True, force=force, form=form)
            for B, H, W in ((2, 3, 4), (5, 1, 1), (11, 13, 13)):      # 1x1: all four borders at once
                c["F%d%s_bias16_b%d_%dx%d" % (ts, tag, B, H, W)] = _ocase(ts=ts, B=B, H=H, W=W, bias16=True, force=force, form=form)
    c["F6_forced_coop6"] = _ocase(ts=6, B=11, H=13, W=13, pool=2, slope=0.5, force=2, form="coop6")
    big = dict(ts=6, B=11, H=13, W=13, slope=0.5, big=True)
    c["F6_tpi6_at_196608_pairs"] = _ocase(N=4016, form="tpi6", threads=256, **big)
    c["F6_coop6_below_196608_pairs"] = _ocase(N=4012, form="coop6", threads=256, **big)
    return c


OUTPUT_CASES = _output_cases()


def output_data(name):
    """M' [P, Mt, N] integers (float32), bias [N] or None, bias16 [16, N] or None; the geometry they are made for"""
    k = OUTPUT_CASES[name]
    geo = wr.geometry(k["ts"], k["B"], k["H"], k["W"], k["pool"] != 0, k["mosaic"])
    rs = np.random.RandomState(_seed("out/" + name))
    mx = M_MAX[k["ts"]]
    m = rs.randint(-mx, mx + 1, size=((k["ts"] + 2) ** 2, geo["Mt"], k["N"])).astype(np.float32)
    bias = rs.randint(-BIAS_MAX, BIAS_MAX + 1, size=k["N"]).astype(np.float32) if k["bias"] else None
    bias16 = rs.randint(-BIAS16_MAX, BIAS16_MAX + 1, size=(16, k["N"])).astype(np.float32) if k["bias16"] else None
    return geo, m, bias, bias16


def output_expected(name, dtype=np.float64, order=None):
    """(full-resolution output or None, pooled output or None, max |x| of what is stored), for the case's pool mode 0 / 1 / 2"""
    k = OUTPUT_CASES[name]
    geo, m, bias, bias16 = output_data(name)
    full = wr.output_transform(m, k["ts"], geo, k["B"], k["H"], k["W"], bias, bias16, k["slope"], dtype, order)
    pooled = wr.pool2(full) if k["pool"] else None
    return (full if k["pool"] != 1 else None), pooled, wr.amax(pooled if k["pool"] else full)


# ---- the ConvLSTM gate transform ----
GATE_FORMS = {6: "gates6", 4: "gates4", 2: "gates2"}
# |h - h64| and |c - c64| bars of the cases that are not bit for bit: 4 x the largest difference between gate_update in float32 numpy and in
# float64 on the case's own inputs (the factor: the device tanhf rounds differently).  Measured baselines (test_wino_transform_cpu.py prints
# and bounds them): h, saturated cases 4.97e-08 (c is exact);  h / c, soft cases 1.81e-07 / 3.42e-07
GATE_H_TOL_SAT = 4 * 4.97e-08
GATE_H_TOL_SOFT = 4 * 1.81e-07
GATE_C_TOL_SOFT = 4 * 3.42e-07


def _gate_cases():
    c = {}
    for ts in (2, 4, 6):
        for U in (32, 96):
            for gname in ("b11_13x13", "one_7x5"):
                B, H, W, _, _ = GEOS[gname]
                for mode in ("sat", "soft"):
                    wide = U == 96
                    c["F%d_U%d_%s_%s" % (ts, U, gname, mode)] = dict(ts=ts, B=B, H=H, W=W, U=U, mode=mode, form=GATE_FORMS[ts], cap=False,
                                                                   xp_ld=4 * U + (4 if wide else 0), c_ld=U + (4 if wide else 0), h_ld=U + (8 if wide else 0))
        c["F%d_U32_cap" % ts] = dict(ts=ts, B=11, H=13, W=13, U=32, mode="sat", form=GATE_FORMS[ts], cap=True, xp_ld=128, c_ld=32, h_ld=32)
    return c


GATE_CASES = _gate_cases()


def gate_data(name):
    """M' [P, Mt, 4U] integers, xproj [B, H, W, 4U] and cstate [B, H, W, U] dyadic, and z = At m A + xproj as the case DESIGNS it:
    sat:  gate pre-activations in {-4, 0, 3} (hard_sigmoid = 0, 0.5, 1 exactly), candidate in {-24, -20, 20, 24} (tanh = -1, 1 in float32 AND in float64),
          c in halves: c_new = f c + i tanh(z_c) is exact;
    soft: everything in eighths within [-3, 3], c in sixteenths within [-2, 2]."""
    k = GATE_CASES[name]
    ts, B, H, W, U = k["ts"], k["B"], k["H"], k["W"], k["U"]
    geo = wr.geometry(ts, B, H, W, False, 0)
    rs = np.random.RandomState(_seed("gates/" + name))
    mx = M_MAX[ts]
    m = rs.randint(-mx, mx + 1, size=((ts + 2) ** 2, geo["Mt"], 4 * U)).astype(np.float32)
    y = wr.frames_from_tiles(wr.tile_outputs(m, ts), ts, geo, B, H, W)
    col = wr.gate_columns(U)
    z = np.empty((B, H, W, 4 * U), dtype=np.float64)
    if k["mode"] == "sat":
        for g in (0, 1, 3):
            z[..., col[g]] = rs.choice([-4.0, 0.0, 3.0], size=(B, H, W, U))
        z[..., col[2]] = rs.choice([-24.0, -20.0, 20.0, 24.0], size=(B, H, W, U))
        c = rs.randint(-8, 9, size=(B, H, W, U)) / 2.0
    else:
        z[...] = rs.randint(-24, 25, size=z.shape) / 8.0
        c = rs.randint(-32, 33, size=(B, H, W, U)) / 16.0
    xproj = z - y
    return geo, m, xproj, c, z
