"""GPU suite: every kernel of csrc/winograd.hip ALONE -- no GEMM between the transforms -- against the float64 reference of
tests/wino_transform_ref.py, with `array_equal`.

The layer tests see these kernels through input transform, GEMM and output transform together, at bars relative to the output's largest value
(2e-4 for F(6x6)): G of F(6x6) holds 2/9, 1/90 ..., so no layer result is exact.  Bt and At hold dyadic rationals only, so each transform taken
alone IS exact in float32 on small integers, in any order of operations (tests/test_wino_transform_cpu.py proves it on every case's own data),
and so are the split forms of V: three bf16 terms hold any float32, two fp16 terms of the scaled V hold 22 bits.  A misplaced tap, a separator
read as data, one wrong coefficient, a lost `lo` term or a row factor off by a power of two cannot pass.

The library's test entries dt_wino_input / dt_wino_output run the production geometry rule and the production launchers on caller buffers and
report WHICH KERNEL the launcher chose, with what grid; every case asserts it, so a moved threshold fails here instead of moving coverage.
Buffers are pre-filled with a NaN bit pattern and carry a guard behind their end: every word a kernel does not own must keep the pattern
(pad rows Mt .. Mp-1 of the split layouts, columns N .. ld-1, the dropped row / column of an odd pooled frame, pixels outside a frame), and
every word it owns must not.  Zeros compare equal whatever their sign.

form -> cases (wino_transform_cases.py):
  input   tpi2, tpi4   f32_F2_* / f32_F4_* (256 threads: *_256_threads_at_131072)      tpi6   f32_F6_forced_tpi6*, f32_F6_tpi6_at_196608_pairs
          coop6        f32_F6_*                      tpi4_s3  tpi4_s3_*                  s3_6 / s3_4 / h2_6 / h2_4   the cases of that name
  output  tpi2, tpi4   F2_* / F4_*                   coop6    F6_* without _tpi6        tpi6   F6_tpi6_*, F6_tpi6_at_196608_pairs
          gates6 / gates4 / gates2   test_gates F6_* / F4_* / F2_*
*_cap cases repeat a case under a workgroup cap (WinoArgs::wg_cap) that makes the kernel's grid-stride loop run three passes, the last one
ragged: the same bits must come out."""
import numpy as np
import pytest
import torch

import mi355_dt
import wino_transform_cases as wc
import wino_transform_ref as wr

pytestmark = pytest.mark.gpu

S32 = np.uint32(wc.SENTINEL32)
S16 = np.uint16(wc.SENTINEL16)
S16X2 = np.uint32(wc.SENTINEL16 | wc.SENTINEL16 << 16)      # the split layouts' buffers: the 16-bit pattern in both halves of a word
POISON = 1.0e6      # what lies between and behind the input's rows: a word read from there cannot give an integer of the expected size


@pytest.fixture(autouse=True)
def _policy_env(monkeypatch):
    for k in ("DT_PIN", "DT_WINO_MOSAIC"):
        monkeypatch.delenv(k, raising=False)


def _mosaic_env(monkeypatch, mosaic):
    if mosaic:
        monkeypatch.setenv("DT_WINO_MOSAIC", str(mosaic))


def _geo_part(g):
    return {k: g[k] for k in ("g", "ph", "pw", "th", "tw", "Mt", "Mp")}


def _three_pass_cap(grid):
    """a workgroup cap under which a grid of `grid` workgroups takes three passes, the last one ragged"""
    for cap in range((grid - 1) // 2, 0, -1):
        if -(-grid // cap) >= 3 and grid % cap:
            return cap
    raise AssertionError("a launch of %d workgroups is too small for a capped case" % grid)


class _Buf(object):
    """A device buffer of 32-bit words: `n` words of payload pre-filled with the sentinel, a guard of `guard` words behind them"""

    def __init__(self, ctx, n, guard, fill=None):
        self.n, self.guard = n, guard
        self.t = torch.empty(n + guard, dtype=torch.int32, device=ctx.device)
        self.t.fill_(int(np.int32(S32.view(np.int32)) if fill is None else fill))

    def f32(self):
        return self.t.view(torch.float32)

    def words(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(np.uint32)


def _nhwc(buf, B, H, W, C, ld, bs=None):
    """the [B, H, W, C] view of a buffer whose pixels are ld floats and whose frames are bs floats apart"""
    bs = H * W * ld if bs is None else bs
    return buf.f32().as_strided((B, H, W, C), (bs, W * ld, ld, 1))


def _check_owned(got_words, want, owned_index, what):
    """got_words: the whole buffer as uint32, guard included.  The words at owned_index (an index into a view of the payload) must equal `want` as
    float32 values; every other word must still hold the sentinel."""
    mask = np.zeros(got_words.shape, dtype=bool)
    view, idx = owned_index(mask)
    view[idx] = True
    got = got_words.view(np.float32)
    gview, _ = owned_index(got)
    want32 = np.asarray(want, dtype=np.float64).astype(np.float32)
    g = gview[idx]
    assert g.shape == want32.shape, (what, g.shape, want32.shape)
    if not np.array_equal(g, want32):
        bad = np.argwhere(g != want32)
        i = tuple(bad[0])
        pytest.fail("%s: %d of %d values differ; first at %s: got %r expected %r" % (what, len(bad), g.size, i, float(g[i]), float(want32[i])))
    stray = np.flatnonzero(got_words[~mask] != S32)
    assert stray.size == 0, "%s: %d words outside what the kernel owns were written (first: word %d of those)" % (what, stray.size, int(stray[0]))


# ================================================================================================ input transform
def _upload_input(ctx, x, ld, bs_extra):
    B, H, W, C = x.shape
    ld = ld or C
    bs = H * W * ld + bs_extra
    buf = _Buf(ctx, B * bs, bs, fill=int(np.float32(POISON).view(np.int32)))
    view = _nhwc(buf, B, H, W, C, ld, bs)
    view.copy_(torch.from_numpy(x).to(ctx.device))
    return buf, view


def _run_input(ctx, k, view, geo, nt, force, cap):
    P = (k["ts"] + 2) ** 2
    n_words = P * nt * geo["Mp"] * k["C"] // 2 if nt else P * geo["Mt"] * k["C"]
    v = _Buf(ctx, n_words, 4096, fill=int(S16X2.view(np.int32)) if nt else None)
    got_geo = ctx.wino_input(view, v.t[:n_words], k["ts"], nt=nt, pooled=k["pooled"], force_form=force, wg_cap=cap)
    return v, got_geo


def _check_input(k, name, v, geo, x, what):
    ts, C, Mt, Mp = k["ts"], k["C"], geo["Mt"], geo["Mp"]
    P = (ts + 2) ** 2
    want = wr.input_transform(x, ts, geo)
    words = v.words()
    if k["nt"] == 0:
        _check_owned(words, want, lambda a: (a[:v.n].reshape(P, Mt, C), Ellipsis), what)
        return
    assert np.all(words[v.n:] == S16X2), what + ": guard words written"
    got = words[:v.n].view(np.uint16).reshape(P, k["nt"], C // 16, Mp, 16)
    assert np.all(got[:, :, :, Mt:] == S16), what + ": pad rows Mt .. Mp-1 written"
    want32 = want.astype(np.float32)
    if k["nt"] == 3:
        ref = wr.pack_bf16x3(want32, Mp, wc.SENTINEL16)
        assert np.array_equal(wr.unpack_bf16x3(got, Mt), want), what + ": the three bf16 terms do not add up to V"
        assert np.array_equal(wr.bf16_value(got[:, :, :, :Mt]), wr.bf16_value(ref[:, :, :, :Mt])), what + ": a term differs from h, m, l of the reference split"
    else:
        am = np.abs(x).max()
        ref = wr.pack_f16x2(want32, ts, am, Mp, wc.SENTINEL16)
        g16, r16 = got[:, :, :, :Mt].view(np.float16), ref[:, :, :, :Mt].view(np.float16)
        for t, term in enumerate(("hi = f16(x s)", "lo = f16(x s - hi)")):
            if not np.array_equal(g16[:, t], r16[:, t]):
                bad = np.argwhere(g16[:, t] != r16[:, t])
                p, cb, tile, cl = bad[0]
                pytest.fail("%s: term %s differs in %d of %d words; first at position %d (xi %d, nu %d), tile %d, channel %d: got %r expected %r"
                            % (what, term, len(bad), g16[:, t].size, p, p // (ts + 2), p % (ts + 2), tile, cb * 16 + cl, float(g16[p, t, cb, tile, cl]),
                               float(r16[p, t, cb, tile, cl])))
        assert np.array_equal(wr.unpack_f16x2(got, ts, am, Mt), want), what + ": the two fp16 terms do not add up to V"


@pytest.mark.parametrize("name", list(wc.INPUT_CASES))
def test_input_transform(ctx, monkeypatch, name):
    k = wc.INPUT_CASES[name]
    _mosaic_env(monkeypatch, k["mosaic"])
    x = wc.input_data(name)
    geo = wr.geometry(k["ts"], k["B"], k["H"], k["W"], k["pooled"], k["mosaic"])
    assert ctx.wino_geometry(k["ts"], k["B"], k["H"], k["W"], k["pooled"]) == _geo_part(geo), "the library's geometry rule and the reference's disagree"
    buf, view = _upload_input(ctx, x, k["ld"], k["bs_extra"])
    v, got = _run_input(ctx, k, view, geo, k["nt"], k["force"], 0)
    assert _geo_part(got) == _geo_part(geo)
    assert got["form"] == mi355_dt.WIN_FORMS[k["form"]], "launch_wino_input took form %d, the case is about %s" % (got["form"], k["form"])
    if k["threads"]:
        assert got["threads"] == k["threads"], got
    if k["nt"] == 2:
        assert ctx.amax_read(57) == np.float32(np.abs(x).max())
    if k["cap"]:      # the same launch under a cap: three passes of the grid-stride loop, the last one ragged
        cap = _three_pass_cap(got["grid"])
        v, capped = _run_input(ctx, k, view, geo, k["nt"], k["force"], cap)
        assert capped["form"] == got["form"] and capped["threads"] == got["threads"] and capped["grid"] == cap, (got, capped)
    _check_input(k, name, v, geo, x, name)


# ================================================================================================ output transform, plain epilogue
def _run_output(ctx, k, geo, m, bias, bias16, cap):
    ts, B, H, W, N = k["ts"], k["B"], k["H"], k["W"], k["N"]
    m_ld, out_ld, out2_ld = k["m_ld"] or N, k["out_ld"] or N, k["out2_ld"] or N
    P = (ts + 2) ** 2
    md = torch.full((P, geo["Mt"], m_ld), POISON, dtype=torch.float32, device=ctx.device)
    md[:, :, :N] = torch.from_numpy(m).to(ctx.device)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(ctx.device)
    out = _Buf(ctx, B * H * W * out_ld, H * W * out_ld) if k["pool"] != 1 else None
    out2 = _Buf(ctx, B * (H // 2) * (W // 2) * out2_ld, max(1, (H // 2) * (W // 2)) * out2_ld) if k["pool"] else None
    got = ctx.wino_output(md, N, B, H, W, ts, bias=dev(bias), bias16=dev(bias16), slope=k["slope"], out=None if out is None else _nhwc(out, B, H, W, N, out_ld),
                          out2=None if out2 is None else _nhwc(out2, B, H // 2, W // 2, N, out2_ld), publish=True, force_form=k["force"], wg_cap=cap)
    return out, out2, got, ctx.amax_read(57)


@pytest.mark.parametrize("name", list(wc.OUTPUT_CASES))
def test_output_transform(ctx, monkeypatch, name):
    k = wc.OUTPUT_CASES[name]
    _mosaic_env(monkeypatch, k["mosaic"])
    ts, B, H, W, N = k["ts"], k["B"], k["H"], k["W"], k["N"]
    geo, m, bias, bias16 = wc.output_data(name)
    full, pooled, am = wc.output_expected(name)
    out, out2, got, got_am = _run_output(ctx, k, geo, m, bias, bias16, 0)
    assert _geo_part(got) == _geo_part(geo)
    assert got["form"] == mi355_dt.WOUT_FORMS[k["form"]], "launch_wino_output took form %d, the case is about %s" % (got["form"], k["form"])
    if k["threads"]:
        assert got["threads"] == k["threads"], got
    if k["cap"]:
        cap = _three_pass_cap(got["grid"])
        out, out2, capped, got_am = _run_output(ctx, k, geo, m, bias, bias16, cap)
        assert capped["form"] == got["form"] and capped["threads"] == got["threads"] and capped["grid"] == cap, (got, capped)
    if out is not None:
        ld = k["out_ld"] or N
        _check_owned(out.words(), full, lambda a: (a[:out.n].reshape(B, H, W, ld), (Ellipsis, slice(0, N))), name + " full-resolution output")
    if out2 is not None:
        ld = k["out2_ld"] or N
        _check_owned(out2.words(), pooled, lambda a: (a[:out2.n].reshape(B, H // 2, W // 2, ld), (Ellipsis, slice(0, N))), name + " pooled output")
    assert got_am == am, "published max |x| %r, the stored values' is %r" % (got_am, am)


# ================================================================================================ the bit-identity claim of DESIGN.md
@pytest.mark.parametrize("B,H,W,pooled", [(11, 13, 13, False), (5, 8, 14, True)], ids=["mosaic", "pooled"])
def test_cooperative_f6_kernels_are_bit_identical_to_thread_per_item(ctx, B, H, W, pooled):
    """random float32 data (no integers: every rounding counts): the lane-cooperative F(6x6) kernels and the one-thread-per-item kernels give the same bits"""
    rs = np.random.RandomState(B * 100 + H)
    C = N = 24
    geo = wr.geometry(6, B, H, W, pooled, 0)
    x = torch.from_numpy((rs.randn(B, H, W, C) * np.exp(rs.randn(B, H, W, C))).astype(np.float32)).to(ctx.device)
    res = {}
    for force, form in ((1, "tpi6"), (2, "coop6")):
        v = torch.zeros(64, geo["Mt"], C, dtype=torch.float32, device=ctx.device)
        got = ctx.wino_input(x, v, 6, nt=0, pooled=pooled, force_form=force)
        assert got["form"] == mi355_dt.WIN_FORMS[form] and got["Mt"] == geo["Mt"]
        res[form] = v.view(torch.int32).cpu().numpy()
    assert np.array_equal(res["tpi6"], res["coop6"]), "input transform: %d words differ" % int((res["tpi6"] != res["coop6"]).sum())
    assert np.isfinite(res["tpi6"].view(np.float32)).all() and np.abs(res["tpi6"].view(np.float32)).max() > 1.0
    m = torch.from_numpy((rs.randn(64, geo["Mt"], N) * np.exp(rs.randn(64, geo["Mt"], N))).astype(np.float32)).to(ctx.device)
    bias = torch.from_numpy(rs.randn(N).astype(np.float32)).to(ctx.device)
    res = {}
    for force, form in ((1, "tpi6"), (2, "coop6")):
        out = torch.zeros(B, H, W, N, dtype=torch.float32, device=ctx.device)
        out2 = torch.zeros(B, H // 2, W // 2, N, dtype=torch.float32, device=ctx.device) if pooled else None
        got = ctx.wino_output(m, N, B, H, W, 6, bias=bias, slope=0.1, out=out, out2=out2, publish=True, force_form=force)
        assert got["form"] == mi355_dt.WOUT_FORMS[form]
        res[form] = [out.view(torch.int32).cpu().numpy(), None if out2 is None else out2.view(torch.int32).cpu().numpy(), ctx.amax_read(57)]
    assert np.array_equal(res["tpi6"][0], res["coop6"][0]), "output transform: %d words differ" % int((res["tpi6"][0] != res["coop6"][0]).sum())
    assert pooled == (res["tpi6"][1] is not None) and (not pooled or np.array_equal(res["tpi6"][1], res["coop6"][1]))
    assert res["tpi6"][2] == res["coop6"][2] and res["tpi6"][2] > 0
    assert np.abs(res["tpi6"][0].view(np.float32)).max() > 1.0


# ================================================================================================ ConvLSTM gate transform
@pytest.mark.parametrize("name", list(wc.GATE_CASES))
def test_gates(ctx, name):
    k = wc.GATE_CASES[name]
    ts, B, H, W, U = k["ts"], k["B"], k["H"], k["W"], k["U"]
    N = 4 * U
    geo, m, xproj, c, z = wc.gate_data(name)
    c64, h64 = wr.gate_update(z, c)
    md = torch.from_numpy(m).to(ctx.device)
    xp = _Buf(ctx, B * H * W * k["xp_ld"], H * W * k["xp_ld"], fill=int(np.float32(POISON).view(np.int32)))
    _nhwc(xp, B, H, W, N, k["xp_ld"]).copy_(torch.from_numpy(xproj.astype(np.float32)).to(ctx.device))

    def run(cap):
        cs = _Buf(ctx, B * H * W * k["c_ld"], H * W * k["c_ld"])
        _nhwc(cs, B, H, W, U, k["c_ld"]).copy_(torch.from_numpy(c.astype(np.float32)).to(ctx.device))
        hb = _Buf(ctx, B * H * W * k["h_ld"], H * W * k["h_ld"])
        got = ctx.wino_output(md, N, B, H, W, ts, out=_nhwc(hb, B, H, W, U, k["h_ld"]), xproj=_nhwc(xp, B, H, W, N, k["xp_ld"]),
                              cstate=_nhwc(cs, B, H, W, U, k["c_ld"]), wg_cap=cap)
        return cs, hb, got
    cs, hb, got = run(0)
    assert _geo_part(got) == _geo_part(geo) and got["form"] == mi355_dt.WOUT_FORMS[k["form"]], got
    if k["cap"]:
        cap = _three_pass_cap(got["grid"])
        cs, hb, capped = run(cap)
        assert capped["form"] == got["form"] and capped["grid"] == cap
    own_c = lambda a: (a[:cs.n].reshape(B, H, W, k["c_ld"]), (Ellipsis, slice(0, U)))
    own_h = lambda a: (a[:hb.n].reshape(B, H, W, k["h_ld"]), (Ellipsis, slice(0, U)))
    cw, hw = cs.words(), hb.words()
    gc = own_c(cw.view(np.float32))[0][..., :U].astype(np.float64)
    gh = own_h(hw.view(np.float32))[0][..., :U].astype(np.float64)
    dc, dh = np.abs(gc - c64).max(), np.abs(gh - h64).max()
    print("gates %s: |c - c64| %.3g  |h - h64| %.3g" % (name, dc, dh))
    if k["mode"] == "sat":
        _check_owned(cw, c64, own_c, name + " c_out")
        h_tol = wc.GATE_H_TOL_SAT
    else:
        assert np.isfinite(gc).all() and dc <= wc.GATE_C_TOL_SOFT, (name, dc)
        _check_owned(cw, gc, own_c, name + " c_out (sentinels)")
        h_tol = wc.GATE_H_TOL_SOFT
    assert np.isfinite(gh).all() and dh <= h_tol, (name, dh, h_tol)
    _check_owned(hw, gh, own_h, name + " h_out (sentinels)")


# ================================================================================================ what the launchers refuse
def _refused(ctx, call, needle):
    with pytest.raises(mi355_dt.NativeError) as e:
        call()
    assert needle in str(e.value), str(e.value)


def test_refused_arguments_are_dt_err_arg_with_a_message(ctx):
    dev = ctx.device
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    x = f(2, 5, 5, 32)
    big = f(64 * 3 * 256 * 32)
    _refused(ctx, lambda: ctx.wino_input(x, big, 3), "unsupported arguments")                          # ts
    _refused(ctx, lambda: ctx.wino_input(f(2, 4, 4, 6), big, 4), "launcher refuses")                   # C % 4
    _refused(ctx, lambda: ctx.wino_input(f(2, 5, 5, 48), big, 6, nt=3), "launcher refuses")            # bf16 split, F6: C % 32
    _refused(ctx, lambda: ctx.wino_input(f(2, 5, 5, 24), big, 4, nt=3), "launcher refuses")            # bf16 split, F4: C % 16
    _refused(ctx, lambda: ctx.wino_input(f(2, 5, 5, 48), big, 4, nt=2), "launcher refuses")            # fp16 split: C % 32
    _refused(ctx, lambda: ctx.wino_input(x, big, 2, nt=3), "launcher refuses")                         # no split form of F(2x2)
    _refused(ctx, lambda: ctx.wino_input(x, f(64 * 2 * 32 - 1), 6), "the buffer has")                  # V too small (Mt = 2)
    _refused(ctx, lambda: ctx.wino_input(x, big[:36 * 3 * 256 * 32 // 2 - 1], 4, nt=3), "the buffer has")
    m = f(64, 2, 128)
    out, out2 = f(2, 5, 5, 128), f(2, 2, 2, 128)
    _refused(ctx, lambda: ctx.wino_output(f(36, 2, 128), 128, 2, 5, 5, 6, out=out), "the buffer has")  # M' of another tile size
    _refused(ctx, lambda: ctx.wino_output(f(64, 2, 6), 6, 2, 5, 5, 6, out=f(2, 5, 5, 6)), "launcher refuses")      # N % 4
    b16 = f(16, 128)
    _refused(ctx, lambda: ctx.wino_output(m, 128, 2, 5, 5, 6, bias16=b16, slope=0.5, out=out), "launcher refuses")
    _refused(ctx, lambda: ctx.wino_output(m, 128, 2, 5, 5, 6, bias16=b16, out=out, out2=out2), "launcher refuses")
    _refused(ctx, lambda: ctx.wino_output(m, 128, 2, 5, 5, 6, bias16=b16, out2=out2), "launcher refuses")
    m64 = f(64, 2, 64)
    _refused(ctx, lambda: ctx.wino_output(m64, 64, 2, 5, 5, 6, out=f(2, 5, 5, 16), xproj=f(2, 5, 5, 64), cstate=f(2, 5, 5, 16)), "launcher refuses")      # gates: N % 128
    # and the same arguments, mended, pass
    assert ctx.wino_output(m, 128, 2, 5, 5, 6, bias16=b16, out=out)["form"] == mi355_dt.WOUT_FORMS["coop6"]
    assert ctx.wino_input(x, big, 6, nt=3)["form"] == mi355_dt.WIN_FORMS["s3_6"]
