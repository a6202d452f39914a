"""Latency of detection scoring: the two launches of Context.detect_score (dt_detect_match, dt_detect_rank).

    python tools/detect_score_latency.py [--out profiles/detect_score.txt]

Input: a set shaped like the decode output of the bench step -- 1440 frames, cap 845, about 22 boxes per frame, gcap 64, 12 classes
(tests/detect_score_ref.make_scene, seed 1) -- scored at 1 threshold and at the 10 COCO thresholds, and the SAME rows in a
[1440, 64, 8] table (cap 64): the rank sees the same rows in use either way, so the difference between its two times is what the
[B, cap] passes cost (the -1 fill of rank / ctp and the compaction), not the ranking.
Times come from the library's own profile (dt_profile_enable: HIP events around every launch; dt_profile_read "score:detect_match" /
"score:detect_rank"): `--calls` launches per reading, `--reps` readings per variant, the variants interleaved; median, lowest and
highest ms per launch.
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=1440)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import object_tracking_amd      # noqa: F401
    import mi355_dt
    import detect_score_ref as dsr
    from utility.evaluate import COCO_THRESHOLDS

    ctx = mi355_dt.Context()
    B, NC, gcap = a.frames, 12, 64
    s64 = dsr.make_scene(B, 64, gcap, NC, 18, 1)
    assert s64["det_counts"].max() <= 64
    wide = np.zeros((B, 845, 8), dtype=np.float32)
    wide[:, :64] = s64["det_boxes"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ctx.device)
    gt = [dev(s64[k]) for k in ("gt_boxes", "gt_counts", "gt_flags")]
    counts = dev(s64["det_counts"])
    tables = {845: dev(wide), 64: dev(s64["det_boxes"])}
    rows = int(s64["det_counts"].sum())
    variants = [(cap, n_thr) for cap in (845, 64) for n_thr in (1, 10)]
    thr_of = lambda n: (0.5,) if n == 1 else COCO_THRESHOLDS
    call = lambda cap, n: ctx.detect_score(tables[cap], counts, gt[0], gt[1], NC, thresholds=thr_of(n), gt_flags=gt[2])
    first = {}
    for v in variants:                       # warm every shape; the two tables must rank alike
        r = call(*v)
        first[v] = {k: r[k].cpu().numpy() for k in ("ndet", "ntp", "ngt")}
    torch.cuda.synchronize()
    for n in (1, 10):
        assert all(np.array_equal(first[(845, n)][k], first[(64, n)][k]) for k in ("ndet", "ntp", "ngt"))
    times = {(v, tag): [] for v in variants for tag in ("score:detect_match", "score:detect_rank")}
    for _ in range(a.reps):
        for v in variants:
            ctx.profile_reset(); ctx.profile_enable(True)
            for _ in range(a.calls):
                call(*v)
            torch.cuda.synchronize()
            ctx.profile_enable(False)
            for tag in ("score:detect_match", "score:detect_rank"):
                r = ctx.profile_read(tag)
                assert r["launches"] == a.calls, (v, tag, r)
                times[(v, tag)].append(r["ms"] / a.calls)
    lines = ["detection scoring latency on %s: %d frames, %d rows in use (%.1f per frame), gcap %d, %d classes; %d launches per reading, "
             "%d readings, interleaved; ms per launch: median (lowest .. highest)"
             % (torch.cuda.get_device_name(ctx.device), B, rows, rows / float(B), gcap, NC, a.calls, a.reps)]
    for v in variants:
        for tag in ("score:detect_match", "score:detect_rank"):
            t = sorted(times[(v, tag)])
            lines.append("cap %-4d n_thr %-3d %-20s %.4f (%.4f .. %.4f)" % (v[0], v[1], tag, t[len(t) // 2], t[0], t[-1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
