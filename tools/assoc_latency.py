"""Latency of the stateless association entries on the benchmark step's association input, and -- with --parent-lib -- the same
rows from another build of the library in the same process on the same buffers, after asserting that both builds' outputs are
bit-equal row by row.

    python tools/assoc_latency.py [--out profiles/assoc_unified.txt] [--parent-lib path/to/the/parent's/libmi355_dt.so]
                                  [--lib path/to/libmi355_dt.so] [--aa 0.0005]

Input: what one bench step hands to the association -- 48 clips x 30 frames at 416x416 through the tracker calibrated by
bench.build_tracker, decoded at the bench's cap (845) -- at thr 0.3, gain 0.5, min_hits 2.  Two layouts: the register form needs
tcap <= 64 and tcap >= cap, so its rows run on the same boxes repacked to cap = tcap = 64 (the tool checks that no frame holds
more); the LDS-form rows run at cap = tcap = 845.  Rows per layout: dt_associate; dt_associate_mem, dt_associate_motion and
dt_associate_tracks without and with the read-out at max_age 0 / 2 / 8; dt_associate_tracks_match 1 / 2 / 3 at max_age 2.

Times come from the library's own profile (dt_profile_enable: HIP events around every launch; dt_profile_read): `--calls`
back-to-back launches per reading, `--reps` readings per row, the rows (and the two builds) interleaved; the table gives the
median, lowest and highest time per launch.

--lib: the build under measurement (default: the one in this tree).  Giving the parent's library on both sides is the A/A run
that sizes the margin: its largest relative difference between the two sides' medians is the figure to pass as --aa to the real
run, which then marks every row whose median exceeds the parent's by more than twice that figure and exits non-zero if any does.
For the A/A run give --lib a COPY of the parent's file under another name: one path is loaded once, and two contexts of one loaded
code object cannot show what two library files differ by before their code does (where the loader places them).  The tool
refuses the same path on both sides.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Lib(object):
    """one build of the library with a context of its own, through the few entries the measurement needs"""

    def __init__(self, path, stream):
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        self.path = os.path.abspath(path)
        self.lib = L = ctypes.CDLL(self.path)
        L.dt_create.argtypes = [ctypes.POINTER(vp)]
        L.dt_destroy.argtypes = [vp]
        L.dt_set_stream.argtypes = [vp, vp]
        L.dt_profile_enable.argtypes = [vp, ci]
        L.dt_profile_reset.argtypes = [vp]
        L.dt_profile_read.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)] + [ctypes.POINTER(ctypes.c_double)] * 3
        L.dt_associate.argtypes = [vp, vp, vp, ci, ci, ci, cf, vp, vp]
        L.dt_associate_mem.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, vp, vp, vp]
        L.dt_associate_motion.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, cf, vp, vp, vp]
        L.dt_associate_tracks.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, cf, ci, vp, vp, vp, vp, vp, vp, vp]
        L.dt_associate_tracks_match.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, cf, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        self.h = vp()
        assert L.dt_create(ctypes.byref(self.h)) == 0
        assert L.dt_set_stream(self.h, vp(stream)) == 0

    def profile_enable(self, on):
        assert self.lib.dt_profile_enable(self.h, 1 if on else 0) == 0

    def profile_reset(self):
        assert self.lib.dt_profile_reset(self.h) == 0

    def profile_read(self, name):
        n = ctypes.c_int64(0)
        ms, fl, by = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        assert self.lib.dt_profile_read(self.h, name.encode(), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        return dict(launches=n.value, ms=ms.value)

    def close(self):
        self.lib.dt_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_unified.txt"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--aa", type=float, default=None, help="largest relative difference of the A/A run; the margin is twice this")
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--gain", type=float, default=0.5)
    ap.add_argument("--min-hits", type=int, default=2)
    args = ap.parse_args()

    import torch
    import object_tracking_amd      # noqa: F401
    from object_tracking_amd.build import LIB
    import bench
    import mi355_dt

    dev = torch.device("cuda", torch.cuda.current_device())
    frames = bench.make_frames(args.clips, args.T, 416, 416, dev, seed0=42)
    trk, _, _ = bench.build_tracker(416, 416, args.T, 32, frames[:1])
    res = trk.track_clips(frames)
    boxes, counts = res["boxes"].contiguous(), res["counts"].contiguous()
    n, T, cap = counts.shape[0], counts.shape[1], boxes.shape[2]
    assert int(counts.max()) <= 64, "a frame holds %d boxes: the tcap = 64 rows need at most 64" % int(counts.max())
    boxes64 = boxes[:, :, :64].contiguous()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    sides = [("new", Lib(args.lib or LIB, stream))]
    if args.parent_lib:
        assert os.path.realpath(args.parent_lib) != os.path.realpath(args.lib or LIB), "both sides name one file: give --lib a copy"
        sides.insert(0, ("parent", Lib(args.parent_lib, stream)))

    def outputs():
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        return dict(ids=i32(n, T, cap), gaps=i32(n, T, cap), hits=i32(n, T, cap), nids=i32(n),
                    tracks=torch.empty((n, T, cap, mi355_dt.DT_TRACK_FLOATS), dtype=torch.float32, device=dev),
                    tinfo=i32(n, T, cap, mi355_dt.DT_TRACK_INTS), tcounts=i32(n, T))
    out = {name: outputs() for name, _ in sides}      # (a row at cap 64 uses the leading part of each buffer)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    gain, mh = args.gain, args.min_hits

    # rows: (name, layout, profile tag, call(side's Lib, side's outputs) -> status)
    rows = []
    for label, bx, c in (("cap 64", boxes64, 64), ("cap %d" % cap, boxes, cap)):
        rows.append(("dt_associate", label, "associate", lambda l, o, bx=bx, c=c: l.lib.dt_associate(
            l.h, P(bx), P(counts), n, T, c, 0.3, P(o["ids"]), P(o["nids"]))))
        for age in (0, 2, 8):
            rows.append(("dt_associate_mem max_age %d" % age, label, "associate:memory", lambda l, o, bx=bx, c=c, age=age: l.lib.dt_associate_mem(
                l.h, P(bx), P(counts), n, T, c, 0.3, age, c, P(o["ids"]), P(o["nids"]), P(o["gaps"]))))
        for age in (0, 2, 8):
            rows.append(("dt_associate_motion max_age %d" % age, label, "associate:motion", lambda l, o, bx=bx, c=c, age=age: l.lib.dt_associate_motion(
                l.h, P(bx), P(counts), n, T, c, 0.3, age, c, gain, P(o["ids"]), P(o["nids"]), P(o["gaps"]))))
        for ro in (False, True):
            for age in (0, 2, 8):
                rows.append(("dt_associate_tracks max_age %d%s" % (age, "" if ro else ", no read-out"), label, "associate:tracks",
                             lambda l, o, bx=bx, c=c, age=age, ro=ro: l.lib.dt_associate_tracks(
                                 l.h, P(bx), P(counts), n, T, c, 0.3, age, c, gain, mh, P(o["ids"]), P(o["nids"]), P(o["gaps"]), P(o["hits"]),
                                 P(o["tracks"] if ro else None), P(o["tinfo"] if ro else None), P(o["tcounts"] if ro else None))))
        for m in (1, 2, 3):
            rows.append(("dt_associate_tracks_match %d max_age 2" % m, label, "associate:tracks_match", lambda l, o, bx=bx, c=c, m=m: l.lib.dt_associate_tracks_match(
                l.h, P(bx), P(counts), n, T, c, 0.3, 2, c, gain, mh, m, P(o["ids"]), P(o["nids"]), P(o["gaps"]), P(o["hits"]), P(o["tracks"]),
                P(o["tinfo"]), P(o["tcounts"]))))

    # ---- before any timing: every row's outputs, bit for bit, from both builds (buffers prefilled, so what a row leaves alone compares too) ----
    # (this pass is also the warm-up: code objects, function attributes)
    for name, label, _, call in rows:
        for sname, lib in sides:
            for k, t in out[sname].items():
                t.view(torch.int32).fill_(-7)
            assert call(lib, out[sname]) == 0, (name, label, sname)
        torch.cuda.synchronize()
        for sname, _ in sides[1:]:
            for k in out[sname]:
                a, b = out[sides[0][0]][k].view(torch.int32), out[sname][k].view(torch.int32)
                assert torch.equal(a, b), "%s, %s: `%s` differs between %s and %s in %d words" % (
                    name, label, k, sides[0][0], sname, int((a != b).sum()))
    equal_line = ("all %d rows: ids, nids, gaps, hits, tracks, tinfo and tcounts bit-equal between the two builds" % len(rows)
                  if len(sides) > 1 else "one build: nothing compared")

    def timed(lib, o, tag, call):
        lib.profile_reset()
        for _ in range(args.calls):
            rc = call(lib, o)
            assert rc == 0, rc
        r = lib.profile_read(tag)
        assert r["launches"] == args.calls, (tag, r)
        return r["ms"] / args.calls

    for _, lib in sides:
        lib.profile_enable(True)
    times = {(k, sname): [] for k in range(len(rows)) for sname, _ in sides}
    for rep in range(args.reps + 1):      # interleaved, so that a drifting clock touches every row and both builds alike; reading 0 is dropped
        for k, (_, _, tag, call) in enumerate(rows):
            for sname, lib in (sides if rep % 2 == 0 else sides[::-1]):
                ms = timed(lib, out[sname], tag, call)
                if rep:
                    times[(k, sname)].append(ms)
    for _, lib in sides:
        lib.profile_enable(False)
    torch.cuda.synchronize()

    lines = ["association latency on the bench step's input: %d clips x %d frames, cap %d, %.1f boxes per frame (min %d, max %d)" % (
                 n, T, cap, float(counts.float().mean()), int(counts.min()), int(counts.max())),
             "dt_profile_read, %d launches per reading, %d readings, rows and builds interleaved; ms per launch; thr 0.3, gain %g, min_hits %d" % (
                 args.calls, args.reps, gain, mh)]
    lines += ["%-7s %s" % (sname, lib.path) for sname, lib in sides]
    lines += [equal_line, ""]
    med = lambda k, s: sorted(times[(k, s)])[len(times[(k, s)]) // 2]
    worst, outside = 0.0, []
    if len(sides) > 1:
        lines.append("%-44s %-8s %9s %9s %9s | %9s %9s %9s | %8s" % ("row", "layout", "parent", "min", "max", "new", "min", "max", "new/par-1"))
    else:
        lines.append("%-44s %-8s %9s %9s %9s" % ("row", "layout", "median", "min", "max"))
    for k, (name, label, _, _) in enumerate(rows):
        cells = []
        for sname, _ in sides:
            t = times[(k, sname)]
            cells.append("%9.4f %9.4f %9.4f" % (med(k, sname), min(t), max(t)))
        line = "%-44s %-8s %s" % (name, label, " | ".join(cells))
        if len(sides) > 1:
            rel = med(k, "new") / med(k, "parent") - 1.0
            worst = max(worst, abs(rel))
            line += " | %+8.3f%%" % (100.0 * rel)
            if args.aa is not None and rel > 2.0 * args.aa:
                outside.append((name, label, rel))
                line += "  OUTSIDE"
        lines.append(line)
    if len(sides) > 1:
        lines += ["", "largest relative difference between the two sides' medians on any row: %.3f %%" % (100.0 * worst)]
    if args.aa is not None:
        lines.append("margin: new median <= parent median x (1 + 2 x %.5f): %s" % (
            args.aa, "every row inside" if not outside else "%d rows outside" % len(outside)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for _, lib in sides:
        lib.close()
    return 1 if outside else 0


if __name__ == "__main__":
    sys.exit(main())
