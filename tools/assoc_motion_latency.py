"""Latency of the association kernels on the benchmark step's input: dt_associate_motion (track motion) against the parent
commit's dt_associate_mem.

    python tools/assoc_motion_latency.py --parent-lib PATH/libmi355_dt.so [--out profiles/assoc_motion.txt] [--gain 0.5]

Input: what one bench step hands to the association -- 48 clips x 30 frames at 416x416 through the tracker calibrated by
bench.build_tracker, decoded with cap = 845.  Every variant is timed with HIP events around `--calls` back-to-back launches on
one stream (no host work between them), `--reps` times; the table gives the median, lowest and highest time per launch.

The register form needs tcap <= 64, and tcap >= cap, so those rows run on the same boxes repacked to cap = 64 (every frame of
the input must then hold at most 64 boxes; the tool checks it); the LDS-form rows run at cap = tcap = 845.  --parent-lib names a
library built from the parent commit; its dt_associate and dt_associate_mem are timed in the same process, on the same buffers,
interleaved with this commit's.  dt_associate and dt_associate_mem are the same code on both commits: their rows must agree
within their own spread.  The number to judge by is dt_associate_motion against the parent's dt_associate_mem with the same
max_age, tcap and layout.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_motion.txt"))
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--gain", type=float, default=0.5)
    args = ap.parse_args()

    import torch
    import object_tracking_amd      # noqa: F401
    import bench
    import mi355_dt      # noqa: F401

    dev = torch.device("cuda", torch.cuda.current_device())
    frames = bench.make_frames(args.clips, args.T, 416, 416, dev, seed0=42)
    trk, _, _ = bench.build_tracker(416, 416, args.T, 32, frames[:1])
    ctx = trk.model.ctx
    res = trk.track_clips(frames)
    boxes, counts = res["boxes"].contiguous(), res["counts"].contiguous()
    n, T, cap = counts.shape[0], counts.shape[1], boxes.shape[2]
    per_frame = counts.float()
    assert int(counts.max()) <= 64, "a frame holds %d boxes: the tcap = 64 rows need at most 64" % int(counts.max())
    boxes64 = boxes[:, :, :64].contiguous()
    ids = torch.empty((n, T, cap), dtype=torch.int32, device=dev)
    gaps = torch.empty((n, T, cap), dtype=torch.int32, device=dev)
    nids = torch.empty((n,), dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ctx._sync_stream()
    L = ctx.lib
    layouts = ((64, boxes64, 64), (cap, boxes, cap))      # (tcap, boxes, cap): register form, LDS form
    ages = (0, 3, 8)

    variants = []      # (name, layout, callable returning the status)

    def old_entries(lib, h, who):
        for tcap, bx, c in layouts:
            variants.append(("dt_associate, %s" % who, "cap %d" % c, lambda bx=bx, c=c: lib.dt_associate(h, P(bx), P(counts), n, T, c, 0.3, P(ids), P(nids))))
        for tcap, bx, c in layouts:
            for age in ages:
                variants.append(("dt_associate_mem max_age %d tcap %d, %s" % (age, tcap, who), "cap %d" % c,
                                 lambda bx=bx, c=c, age=age, tcap=tcap: lib.dt_associate_mem(h, P(bx), P(counts), n, T, c, 0.3, age, tcap, P(ids), P(nids), P(gaps))))

    PL = ph = None
    if args.parent_lib:
        PL = ctypes.CDLL(os.path.abspath(args.parent_lib))
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        PL.dt_create.argtypes = [ctypes.POINTER(vp)]
        PL.dt_set_stream.argtypes = [vp, vp]
        PL.dt_associate.argtypes = [vp, vp, vp, ci, ci, ci, cf, vp, vp]
        PL.dt_associate_mem.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, vp, vp, vp]
        PL.dt_destroy.argtypes = [vp]
        ph = vp()
        assert PL.dt_create(ctypes.byref(ph)) == 0
        PL.dt_set_stream(ph, st)
        old_entries(PL, ph, "parent commit")
    old_entries(L, ctx.h, "this commit")
    for tcap, bx, c in layouts:
        for age in ages:
            variants.append(("dt_associate_motion max_age %d tcap %d" % (age, tcap), "cap %d" % c,
                             lambda bx=bx, c=c, age=age, tcap=tcap: L.dt_associate_motion(ctx.h, P(bx), P(counts), n, T, c, 0.3, age, tcap, args.gain,
                                                                                           P(ids), P(nids), P(gaps))))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            rc = fn()
            assert rc == 0, rc
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.calls

    for _, _, fn in variants:      # warm-up: code objects, function attributes
        timed(fn)
    times = [[] for _ in variants]
    for _ in range(args.reps):      # interleaved, so that a drifting clock touches every row alike
        for k, (_, _, fn) in enumerate(variants):
            times[k].append(timed(fn))
    torch.cuda.synchronize()

    lines = ["association latency on the bench step's input: %d clips x %d frames, cap %d, %.1f boxes per frame (min %d, max %d)" % (
                 n, T, cap, float(per_frame.mean()), int(counts.min()), int(counts.max())),
             "HIP events around %d back-to-back launches, %d repetitions, rows interleaved; ms per launch; motion gain %g" % (args.calls, args.reps, args.gain),
             "",
             "%-56s %-8s %9s %9s %9s" % ("variant", "layout", "median", "min", "max")]
    med = {}
    for (name, layout, _), t in zip(variants, times):
        t = sorted(t)
        med[(name, layout)] = t[len(t) // 2]
        lines.append("%-56s %-8s %9.4f %9.4f %9.4f" % (name, layout, t[len(t) // 2], t[0], t[-1]))
    lines.append("")
    who = "parent commit" if args.parent_lib else "this commit"
    lines.append("dt_associate_motion against dt_associate_mem of the %s, same max_age, tcap and layout (the margin it was sized with: +25 %%):" % who)
    for tcap, _, c in layouts:
        for age in ages:
            base = med[("dt_associate_mem max_age %d tcap %d, %s" % (age, tcap, who), "cap %d" % c)]
            v = med[("dt_associate_motion max_age %d tcap %d" % (age, tcap), "cap %d" % c)]
            lines.append("  max_age %d tcap %-4d %-8s ratio %.3f (%+6.1f %%)" % (age, tcap, "cap %d" % c, v / base, 100.0 * (v / base - 1.0)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if args.parent_lib:
        PL.dt_destroy(ph)


if __name__ == "__main__":
    main()
