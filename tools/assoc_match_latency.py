"""Latency of the track match policies (dt_associate_tracks_match, match 1 / 2 / 3) against match 0, and of dt_associate_tracks
against the same entry of another build of the library, on the benchmark step's association input.

    python tools/assoc_match_latency.py [--out profiles/assoc_match.txt] [--baseline-lib path/to/another/libmi355_dt.so]

Input: what one bench step hands to the association -- 48 clips x 30 frames at 416x416 through the tracker calibrated by
bench.build_tracker, decoded at the bench's cap (845) -- with max_age 2, gain 0.5, min_hits 2.  Times come from the library's own
profile (dt_profile_enable: HIP events around every launch; dt_profile_read): `--calls` launches per reading, `--reps` readings per
variant, the variants interleaved; the table gives the median, lowest and highest time per launch.

The register form needs tcap <= 64, and tcap >= cap, so those rows run on the same boxes repacked to cap = 64 (the tool checks
that no frame holds more); the LDS-form rows run at cap = tcap = 845.  `no read-out` rows pass NULL for d_tracks / d_tinfo /
d_tcounts.  The bench input is sparse (22.5 boxes per frame); the `dense` rows run the LDS form on a synthetic scene of 140 objects
per frame (15 % missed, 5 % label flips per frame: the density of the tests' lds_form case), the case the best-first order's
rescans are sized for.

--baseline-lib: a libmi355_dt.so built from another commit (the parent's).  Its dt_associate_tracks runs in the same process on
the same buffers, interleaved with this build's, through a context of its own; rows named `baseline`.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_MS = 83.5      # the bench step the shares are quoted against


def dense_scene(n_clips, T, cap, n_obj, seed):
    """moving boxes with births, deaths and label flips, as the tests' generator draws them: [n_clips, T, cap, 8], [n_clips, T]"""
    import numpy as np
    boxes = np.zeros((n_clips, T, cap, 8), dtype=np.float32)
    counts = np.zeros((n_clips, T), dtype=np.int32)
    for k in range(n_clips):
        rs = np.random.RandomState(seed + k)
        pos = rs.rand(n_obj, 2); vel = (rs.rand(n_obj, 2) - .5) * .06; wh = rs.rand(n_obj, 2) * .2 + .05
        lab = rs.randint(0, 3, n_obj)
        for t in range(T):
            alive = [j for j in range(n_obj) if rs.rand() > 0.15]
            rs.shuffle(alive)
            for i, j in enumerate(alive[:cap]):
                p = pos[j] + vel[j] * t
                boxes[k, t, i] = [p[0], p[1], wh[j, 0], wh[j, 1], .9, lab[j] if rs.rand() > .05 else (lab[j] + 1) % 3, .8, i]
            counts[k, t] = min(len(alive), cap)
    return boxes, counts


class Baseline(object):
    """another build of the library, through the few entries the measurement needs"""

    def __init__(self, path, stream):
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        self.lib = L = ctypes.CDLL(os.path.abspath(path))
        L.dt_create.argtypes = [ctypes.POINTER(vp)]
        L.dt_destroy.argtypes = [vp]
        L.dt_set_stream.argtypes = [vp, vp]
        L.dt_profile_enable.argtypes = [vp, ci]
        L.dt_profile_reset.argtypes = [vp]
        L.dt_profile_read.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)] + [ctypes.POINTER(ctypes.c_double)] * 3
        L.dt_associate_tracks.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, cf, ci, vp, vp, vp, vp, vp, vp, vp]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_match.txt"))
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--clips", type=int, default=48)
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--max-age", type=int, default=2)
    ap.add_argument("--gain", type=float, default=0.5)
    ap.add_argument("--min-hits", type=int, default=2)
    ap.add_argument("--dense-objects", type=int, default=140)
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
    db, dc = dense_scene(n, T, cap, args.dense_objects, seed=7)
    dboxes, dcounts = torch.from_numpy(db).to(dev), torch.from_numpy(dc).to(dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    ids, gaps, hits, nids = i32(n, T, cap), i32(n, T, cap), i32(n, T, cap), i32(n)
    tracks = torch.empty((n, T, cap, mi355_dt.DT_TRACK_FLOATS), dtype=torch.float32, device=dev)
    tinfo, tcounts = i32(n, T, cap, mi355_dt.DT_TRACK_INTS), i32(n, T)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ctx._sync_stream()
    L, h = ctx.lib, ctx.h
    base = Baseline(args.baseline_lib, torch.cuda.current_stream(dev).cuda_stream) if args.baseline_lib else None
    age, gain, mh = args.max_age, args.gain, args.min_hits
    # (label, boxes, counts, cap = tcap)
    layouts = (("cap 64", boxes64, counts, 64), ("cap %d" % cap, boxes, counts, cap), ("dense", dboxes, dcounts, cap))

    variants = []      # (name, layout, owner of the profile, profile tag, callable returning the status)
    for label, bx, ct, c in layouts:
        for ro in ((False, True) if label != "dense" else (True,)):
            out3 = (tracks, tinfo, tcounts) if ro else (None, None, None)
            suffix = "" if ro else ", no read-out"
            if base is not None:
                variants.append(("baseline dt_associate_tracks" + suffix, label, base, "associate:tracks",
                                 lambda bx=bx, ct=ct, c=c, o=out3: base.lib.dt_associate_tracks(
                                     base.h, P(bx), P(ct), n, T, c, 0.3, age, c, gain, mh, P(ids), P(nids), P(gaps), P(hits), P(o[0]), P(o[1]), P(o[2]))))
            variants.append(("dt_associate_tracks" + suffix, label, ctx, "associate:tracks",
                             lambda bx=bx, ct=ct, c=c, o=out3: L.dt_associate_tracks(
                                 h, P(bx), P(ct), n, T, c, 0.3, age, c, gain, mh, P(ids), P(nids), P(gaps), P(hits), P(o[0]), P(o[1]), P(o[2]))))
            for m in (1, 2, 3):
                variants.append(("dt_associate_tracks_match match %d" % m + suffix, label, ctx, "associate:tracks_match",
                                 lambda bx=bx, ct=ct, c=c, o=out3, m=m: L.dt_associate_tracks_match(
                                     h, P(bx), P(ct), n, T, c, 0.3, age, c, gain, mh, m, P(ids), P(nids), P(gaps), P(hits), P(o[0]), P(o[1]),
                                     P(o[2]))))

    def timed(owner, tag, fn):
        owner.profile_reset()
        for _ in range(args.calls):
            rc = fn()
            assert rc == 0, rc
        r = owner.profile_read(tag)
        assert r["launches"] == args.calls, (tag, r)
        return r["ms"] / args.calls

    ctx.profile_enable(True)
    if base is not None:
        base.profile_enable(True)
    opened = {}
    for name, label, owner, tag, fn in variants:      # warm-up: code objects, function attributes; and the ids each policy opens
        timed(owner, tag, fn)
        torch.cuda.synchronize()
        opened[(name, label)] = float(nids.float().mean())
    times = [[] for _ in variants]
    for _ in range(args.reps):      # interleaved, so that a drifting clock touches every row alike
        for k, (_, _, owner, tag, fn) in enumerate(variants):
            times[k].append(timed(owner, tag, fn))
    ctx.profile_enable(False)
    if base is not None:
        base.profile_enable(False)
    torch.cuda.synchronize()

    lines = ["association latency on the bench step's input: %d clips x %d frames, cap %d, %.1f boxes per frame (min %d, max %d)" % (
                 n, T, cap, float(counts.float().mean()), int(counts.min()), int(counts.max())),
             "dense: %d objects per clip, %.1f boxes per frame (min %d, max %d), cap = tcap = %d" % (
                 args.dense_objects, float(dcounts.float().mean()), int(dcounts.min()), int(dcounts.max()), cap),
             "dt_profile_read, %d launches per reading, %d readings, rows interleaved; ms per launch; max_age %d, gain %g, min_hits %d" % (
                 args.calls, args.reps, age, gain, mh),
             "baseline: %s" % ("dt_associate_tracks of another build of the library, same process, same buffers" if base else "none given"),
             "",
             "%-58s %-8s %9s %9s %9s %9s" % ("variant", "layout", "median", "min", "max", "ids/clip")]
    med, spread = {}, {}
    for (name, label, _, _, _), t in zip(variants, times):
        t = sorted(t)
        med[(name, label)] = t[len(t) // 2]
        spread[(name, label)] = t[-1] - t[0]
        lines.append("%-58s %-8s %9.4f %9.4f %9.4f %9.1f" % (name, label, t[len(t) // 2], t[0], t[-1], opened[(name, label)]))
    if base is not None:
        lines += ["", "(a) dt_associate_tracks, this build against the baseline: difference of the medians, and the baseline's own spread (max - min)"]
        for label, _, _, _ in layouts:
            for suffix in (", no read-out", ""):
                k0, k1 = ("baseline dt_associate_tracks" + suffix, label), ("dt_associate_tracks" + suffix, label)
                if k0 in med:
                    lines.append("  %-8s %-14s %+.4f ms (%+.2f %%), baseline spread %.4f ms" % (
                        label, suffix[2:] or "read-out", med[k1] - med[k0], 100.0 * (med[k1] / med[k0] - 1.0), spread[k0]))
    lines += ["", "(b) match 1 / 2 / 3 against match 0 (dt_associate_tracks), same layout: ratio, and the difference as a share of the %.1f ms step" % STEP_MS]
    for label, _, _, _ in layouts:
        for suffix in (", no read-out", ""):
            k0 = ("dt_associate_tracks" + suffix, label)
            if k0 not in med:
                continue
            for m in (1, 2, 3):
                v = med[("dt_associate_tracks_match match %d" % m + suffix, label)]
                lines.append("  %-8s %-14s match %d  ratio %.3f  %+.4f ms  (%+.3f %% of the step)" % (
                    label, suffix[2:] or "read-out", m, v / med[k0], v - med[k0], 100.0 * (v - med[k0]) / STEP_MS))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if base is not None:
        base.close()


if __name__ == "__main__":
    main()
