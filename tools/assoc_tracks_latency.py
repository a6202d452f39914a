"""Latency of dt_associate_tracks (track read-out on) against dt_associate_motion on the benchmark step's association input.

    python tools/assoc_tracks_latency.py [--out profiles/assoc_tracks.txt] [--gain 0.5] [--min-hits 2]

Input: what one bench step hands to the association -- 48 clips x 30 frames at 416x416 through the tracker calibrated by
bench.build_tracker, decoded at the bench's cap (845).  Times come from the library's own profile (dt_profile_enable: HIP events
around every launch; dt_profile_read("associate:motion" / "associate:tracks")): `--calls` launches per reading, `--reps` readings
per variant, the variants interleaved; the table gives the median, lowest and highest time per launch.

The register form needs tcap <= 64, and tcap >= cap, so those rows run on the same boxes repacked to cap = 64 (the tool checks
that no frame holds more); the LDS-form rows run at cap = tcap = 845.  The read-out writes tcap rows of 48 bytes per frame, so
at tcap = 845 it is most of the kernel's traffic; `no read-out` rows pass NULL for d_tracks / d_tinfo / d_tcounts.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_tracks.txt"))
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--gain", type=float, default=0.5)
    ap.add_argument("--min-hits", type=int, default=2)
    args = ap.parse_args()

    import torch
    import object_tracking_amd      # noqa: F401
    import bench
    import mi355_dt

    dev = torch.device("cuda", torch.cuda.current_device())
    frames = bench.make_frames(args.clips, args.T, 416, 416, dev, seed0=42)
    trk, _, _ = bench.build_tracker(416, 416, args.T, 32, frames[:1])
    ctx = trk.model.ctx
    res = trk.track_clips(frames)
    boxes, counts = res["boxes"].contiguous(), res["counts"].contiguous()
    n, T, cap = counts.shape[0], counts.shape[1], boxes.shape[2]
    assert int(counts.max()) <= 64, "a frame holds %d boxes: the tcap = 64 rows need at most 64" % int(counts.max())
    boxes64 = boxes[:, :, :64].contiguous()
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    ids, gaps, hits, nids = i32(n, T, cap), i32(n, T, cap), i32(n, T, cap), i32(n)
    tracks = torch.empty((n, T, cap, mi355_dt.DT_TRACK_FLOATS), dtype=torch.float32, device=dev)
    tinfo, tcounts = i32(n, T, cap, mi355_dt.DT_TRACK_INTS), i32(n, T)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ctx._sync_stream()
    L, h = ctx.lib, ctx.h
    layouts = ((64, boxes64, 64), (cap, boxes, cap))      # (tcap, boxes, cap): register form, LDS form
    ages = (0, 2, 8)

    variants = []      # (name, layout, profile tag, callable returning the status)
    for tcap, bx, c in layouts:
        for age in ages:
            variants.append(("dt_associate_motion max_age %d tcap %d" % (age, tcap), "cap %d" % c, "associate:motion",
                             lambda bx=bx, c=c, age=age, tcap=tcap: L.dt_associate_motion(h, P(bx), P(counts), n, T, c, 0.3, age, tcap, args.gain,
                                                                                           P(ids), P(nids), P(gaps))))
            variants.append(("dt_associate_tracks max_age %d tcap %d, no read-out" % (age, tcap), "cap %d" % c, "associate:tracks",
                             lambda bx=bx, c=c, age=age, tcap=tcap: L.dt_associate_tracks(h, P(bx), P(counts), n, T, c, 0.3, age, tcap, args.gain,
                                                                                           args.min_hits, P(ids), P(nids), P(gaps), P(hits),
                                                                                           None, None, None)))
            variants.append(("dt_associate_tracks max_age %d tcap %d" % (age, tcap), "cap %d" % c, "associate:tracks",
                             lambda bx=bx, c=c, age=age, tcap=tcap: L.dt_associate_tracks(h, P(bx), P(counts), n, T, c, 0.3, age, tcap, args.gain,
                                                                                           args.min_hits, P(ids), P(nids), P(gaps), P(hits),
                                                                                           P(tracks), P(tinfo), P(tcounts))))

    def timed(tag, fn):
        ctx.profile_reset()
        for _ in range(args.calls):
            rc = fn()
            assert rc == 0, rc
        r = ctx.profile_read(tag)
        assert r["launches"] == args.calls, (tag, r)
        return r["ms"] / args.calls

    ctx.profile_enable(True)
    for _, _, tag, fn in variants:      # warm-up: code objects, function attributes
        timed(tag, fn)
    times = [[] for _ in variants]
    for _ in range(args.reps):      # interleaved, so that a drifting clock touches every row alike
        for k, (_, _, tag, fn) in enumerate(variants):
            times[k].append(timed(tag, fn))
    ctx.profile_enable(False)
    torch.cuda.synchronize()
    rows = int(tcounts.sum())

    lines = ["association latency on the bench step's input: %d clips x %d frames, cap %d, %.1f boxes per frame (min %d, max %d)" % (
                 n, T, cap, float(counts.float().mean()), int(counts.min()), int(counts.max())),
             "dt_profile_read, %d launches per reading, %d readings, rows interleaved; ms per launch; gain %g, min_hits %d" % (
                 args.calls, args.reps, args.gain, args.min_hits),
             "(the last read-out call, max_age %d at tcap %d, wrote %d rows, %.1f per frame)" % (ages[-1], cap, rows, rows / float(n * T)),
             "",
             "%-56s %-8s %9s %9s %9s" % ("variant", "layout", "median", "min", "max")]
    med = {}
    for (name, layout, _, _), t in zip(variants, times):
        t = sorted(t)
        med[(name, layout)] = t[len(t) // 2]
        lines.append("%-56s %-8s %9.4f %9.4f %9.4f" % (name, layout, t[len(t) // 2], t[0], t[-1]))
    lines.append("")
    lines.append("dt_associate_tracks against dt_associate_motion, same max_age, tcap and layout: without / with the read-out")
    for tcap, _, c in layouts:
        for age in ages:
            base = med[("dt_associate_motion max_age %d tcap %d" % (age, tcap), "cap %d" % c)]
            v0 = med[("dt_associate_tracks max_age %d tcap %d, no read-out" % (age, tcap), "cap %d" % c)]
            v1 = med[("dt_associate_tracks max_age %d tcap %d" % (age, tcap), "cap %d" % c)]
            lines.append("  max_age %d tcap %-4d %-8s ratio %.3f (%+6.1f %%) / %.3f (%+6.1f %%)" % (
                age, tcap, "cap %d" % c, v0 / base, 100.0 * (v0 / base - 1.0), v1 / base, 100.0 * (v1 / base - 1.0)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
