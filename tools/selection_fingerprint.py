"""Which kernel forms the library selects, as a file two trees can be compared by.

    python tools/selection_fingerprint.py --out A.json                 # this tree
    python tools/selection_fingerprint.py --root DIR --out B.json      # another tree (e.g. a checkout of the parent commit, built)
    python tools/selection_fingerprint.py --out A.json --compare B.json

For each policy of POLICIES one fresh child process (one at a time, each under its own timeout; this process never opens the
GPU; the first failing child ends the run) runs, with graphs off and profiling on and synthetic weights: the detector forward
at 416x416 for batch 1 .. 64 and at 608x608 for batch 1, 4, 12, detector_extract of two layers at batch 8 and 16, track_clips for four (clips, T)
and one warm track_stream call.  After each call every profile entry's launches / flops / bytes (not ms) are recorded and the
table is reset.  The batches straddle every default threshold of network.hip's choosers.  --compare: the same names per call,
launches equal, flops and bytes equal to 1e-9 relative; profiles/selection_fingerprint.txt holds the outcome.
"""
import argparse
import json
import os
import subprocess
import sys

POLICIES = ["default", "DT_PIN=1", "DT_S3_H2=0", "DT_S3=0", "DT_WINO=0", "DT_C3H2=0", "DT_C3FUSE=0", "DT_TRK_MERGE=0", "DT_WINO_FUSED4=3"]
DETECT = {416: [1, 2, 4, 8, 11, 12, 16, 20, 32, 64], 608: [1, 4, 12]}
EXTRACT = [("leaky_re_lu_5", 8), ("leaky_re_lu_5", 16), ("leaky_re_lu_20", 8), ("leaky_re_lu_20", 16)]
CLIPS = [(1, 30), (2, 30), (8, 4), (48, 30)]
RTOL = 1e-9


def child(root):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    import object_tracking_amd      # noqa: F401
    from models_tracking.MultiObjDetTracker import MultiObjDetTracker
    from utility import synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    calls = []

    def tracker(size):
        class Trk(MultiObjDetTracker):
            IMAGE_H = IMAGE_W = size
            GRID_H = GRID_W = size // 32
            SEQUENCE_LENGTH = 30
            LOAD_MODEL = False
        C = len(Trk.LABELS)
        trk = Trk(detector_weights=synth.synth_darknet_blob(C, seed=1234), tracker_weights=synth.synth_tracker_weights(C, seed=1235))
        ctx = trk.model.ctx
        ctx.graph_enable(False)
        ctx.profile_reset(); ctx.profile_enable(True)
        return trk, ctx

    def frames(size, n):      # [n, size, size, 3] uint8: rolls of one rendered clip (the selection looks at shapes, not at pixels)
        base = torch.from_numpy(synth.synth_clip(30, size, size, 8, seed=42)).to(dev)
        return torch.stack([torch.roll(base[i % 30], shifts=(17 * (i // 30), 29 * (i // 30)), dims=(0, 1)) for i in range(n)]).contiguous()

    def record(ctx, name, fn):
        fn()
        torch.cuda.synchronize()
        tab = {}
        for nm in ctx.profile_names():
            pr = ctx.profile_read(nm)
            tab[nm] = [pr["launches"], pr["flops"], pr["bytes"]]
        ctx.profile_reset()
        calls.append({"call": name, "table": tab})

    for size, batches in sorted(DETECT.items()):
        trk, ctx = tracker(size)
        x = frames(size, max(max(batches), 48 * 30 if size == 416 else 0))
        for b in batches:
            record(ctx, "detect_%d_b%d" % (size, b), lambda: ctx.detect_forward(x[:b]))
        if size != 416:
            continue
        for layer, b in EXTRACT:
            record(ctx, "extract_%s_b%d" % (layer, b), lambda: ctx.detector_extract(x[:b], layer))
        for n, T in CLIPS:
            clip = x[:n * T].reshape(n, T, size, size, 3)
            record(ctx, "track_clips_%dx%d" % (n, T), lambda: trk.track_clips(clip))
        trk.open_streams(8)
        one = x[:8].reshape(8, 1, size, size, 3)
        trk.track_stream(one, list(range(8)))
        ctx.profile_reset()
        record(ctx, "track_stream_warm_8x1", lambda: trk.track_stream(one, list(range(8))))
    json.dump(calls, sys.stdout)


def compare(a, b):
    lines, bad = [], 0
    for pol in POLICIES:
        ca, cb = a.get(pol), b.get(pol)
        if ca is None or cb is None or [c["call"] for c in ca] != [c["call"] for c in cb]:
            lines.append("%-18s calls differ or policy missing" % pol)
            bad += 1
            continue
        names = diffs = 0
        for x, y in zip(ca, cb):
            for nm in sorted(set(x["table"]) | set(y["table"])):
                names += 1
                u, v = x["table"].get(nm), y["table"].get(nm)
                ok = u is not None and v is not None and u[0] == v[0] and all(abs(p - q) <= RTOL * max(abs(p), abs(q)) for p, q in zip(u[1:], v[1:]))
                if not ok:
                    diffs += 1
                    lines.append("  %s %s %s: %s vs %s" % (pol, x["call"], nm, u, v))
        lines.append("%-18s %d calls, %d names compared, %d differences" % (pol, len(ca), names, diffs))
        bad += diffs
    lines.append("SAME SELECTION" if not bad else "DIFFERENT: %d" % bad)
    return "\n".join(lines), bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", default=None, help="a file written by an earlier run: compare --out (run first unless it exists) against it")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.root)
    if not a.out:
        ap.error("--out is required")
    if not (a.compare and os.path.exists(a.out)):
        res = {}
        for pol in POLICIES:
            env = dict(os.environ)
            if pol != "default":
                k, v = pol.split("=")
                env[k] = v
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", a.root], env=env, timeout=a.timeout,
                               stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.exit("policy %s: child exited with %d" % (pol, r.returncode))
            res[pol] = json.loads(r.stdout[r.stdout.index("[{"):])
            print("%s: %d calls" % (pol, len(res[pol])), flush=True)
            with open(a.out, "w") as f:
                json.dump(res, f)
    if a.compare:
        with open(a.out) as fa, open(a.compare) as fb:
            text, bad = compare(json.load(fa), json.load(fb))
        print(text)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
