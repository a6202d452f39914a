"""Latency of identity scoring (dt_identity_overlap, dt_assign_max) beside track scoring (dt_track_score) on the same data.

    python tools/identity_score_latency.py [--out profiles/identity_score.txt]

Input: the two data sets of tools/track_score_latency.py -- the 48 clips x 30 frames of tests/track_score_ref.make_scene (seeds
100 .. 147, 6 .. 10 objects, cap 16; tables of 32 ground-truth and 96 hypothesis trajectories) and the dense scene of 140 objects
(gcap 128, hcap 160, 8 clips x 8 frames; tables of 256 and 512) -- with dt_assign_max on the overlap each leaves, and one
solver-only point: a single 256 x 256 problem, dense (weights 0 .. 29 at random) and as a clip leaves it (a diagonal of long
overlaps plus 3 % short ones).
Times come from the library's own profile (dt_profile_enable: HIP events around every launch; dt_profile_read): `--calls`
launches per reading, `--reps` readings per variant, the variants interleaved; median, lowest and highest ms per launch.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import object_tracking_amd      # noqa: F401
    import mi355_dt
    import track_score_ref as tsr

    ctx = mi355_dt.Context()
    keys = ("gt_boxes", "gt_counts", "gt_ids", "hyp_boxes", "hyp_counts", "hyp_ids")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ctx.device)
    sparse = [tsr.make_scene(30, 16, 16, 6 + k % 5, 100 + k) for k in range(48)]
    dense = [tsr.make_scene(8, 128, 160, 140, 7 + k) for k in range(8)]
    variants, notes = [], []
    for label, scenes, ocap, acap, bcap in (("48 x 30, cap 16", sparse, 64, 32, 96), ("dense 8 x 8, gcap 128 / hcap 160", dense, 256, 256, 512)):
        d = [dev(np.stack([s[k] for s in scenes])) for k in keys]
        r = ctx.identity_score(*d, gt_cap=acap, hyp_cap=bcap)
        sz = r["sizes"].cpu().numpy()
        notes.append("%s: trajectories per clip gt %d .. %d, hyp %d .. %d, overflow boxes %d, valid pairs %d, IDTP %d"
                     % (label, sz[:, 3].min(), sz[:, 3].max(), sz[:, 4].min(), sz[:, 4].max(), int(sz[:, 5:7].sum()), int(sz[:, 7].sum()),
                        int(r["idtp"].sum())))
        variants.append(("dt_track_score", label, "associate:score", lambda d=d, o=ocap: ctx.track_score(*d, obj_cap=o)))
        variants.append(("dt_identity_overlap (tables %d / %d)" % (acap, bcap), label, "associate:identity_overlap",
                         lambda d=d, ac=acap, bc=bcap: ctx.identity_overlap(*d, gt_cap=ac, hyp_cap=bc)))
        variants.append(("dt_assign_max on its overlap", label, "associate:assign_max",
                         lambda r=r: ctx.assign_max(r["overlap"], r["sizes"], 3, 4)))
    rs = np.random.RandomState(5)
    full = rs.randint(0, 30, size=(1, 256, 256)).astype(np.int32)
    clip = (rs.randint(1, 6, size=(1, 256, 256)) * (rs.rand(1, 256, 256) < 0.03)).astype(np.int32)
    clip[0, np.arange(256), rs.permutation(256)] = rs.randint(10, 30, size=256)
    for name, w in (("dense weights 0 .. 29", full), ("a permuted diagonal of 10 .. 29 plus 3 % of 1 .. 5", clip)):
        w = dev(w)
        variants.append(("dt_assign_max, %s" % name, "solver only, 1 x 256 x 256", "associate:assign_max", lambda w=w: ctx.assign_max(w)))
    for v in variants:                       # warm every shape
        v[3]()
    torch.cuda.synchronize()
    times = {(v[0], v[1]): [] for v in variants}
    for _ in range(a.reps):
        for name, label, tag, call in variants:
            ctx.profile_reset(); ctx.profile_enable(True)
            for _ in range(a.calls):
                call()
            torch.cuda.synchronize()
            ctx.profile_enable(False)
            r = ctx.profile_read(tag)
            assert r["launches"] == a.calls, (name, r)
            times[(name, label)].append(r["ms"] / a.calls)
    lines = ["identity scoring latency: %d launches per reading, %d readings, interleaved; ms per launch: median (lowest .. highest)" % (a.calls, a.reps)]
    for name, label, _, _ in variants:
        t = sorted(times[(name, label)])
        lines.append("%-34s %-66s %.4f (%.4f .. %.4f)" % (label, name, t[len(t) // 2], t[0], t[-1]))
    lines += notes
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
