"""Latency of track scoring (dt_track_score) beside the association that produced the ids it scores.

    python tools/track_score_latency.py [--out profiles/track_score.txt]

Input: the 48 clips x 30 frames of tests/test_gpu_track_score.py::test_48_clips_in_one_call (tests/track_score_ref.make_scene,
seeds 100 .. 147, 6 .. 10 objects, cap 16, object table of 64 rows), and a dense scene of 140 objects (gcap 128, hcap 160, table
of 256 rows, 8 clips x 8 frames).  dt_associate_tracks_match runs on the same hypothesis boxes with the tracker settings of the
scenes (best-IoU-first, max_age 1), without read-out, in its register form (tcap = cap) and in its LDS form (tcap = 80 / 512).
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
    trk = tsr.TRACKER
    variants = []
    for label, scenes, ocap, tcap_lds in (("48 x 30, cap 16", sparse, 64, 80), ("dense 8 x 8, gcap 128 / hcap 160", dense, 256, 512)):
        d = [dev(np.stack([s[k] for s in scenes])) for k in keys]
        hcap = d[3].shape[2]
        variants.append(("dt_track_score", label, "associate:score", lambda d=d, o=ocap: ctx.track_score(*d, obj_cap=o)))
        variants.append(("dt_track_score, no per-row outputs", label, "associate:score",
                         lambda d=d, o=ocap: ctx.track_score(*d, obj_cap=o, per_box=False)))
        for tcap in ((hcap, tcap_lds) if hcap <= 64 else (tcap_lds,)):
            variants.append(("dt_associate_tracks_match tcap %d (%s form)" % (tcap, "register" if tcap <= 64 else "LDS"), label,
                             "associate:tracks_match",
                             lambda d=d, tc=tcap: ctx.associate_tracks(d[3], d[4], trk["thr"], trk["max_age"], trk["gain"], trk["min_hits"],
                                                                       track_cap=tc, match=trk["match"], readout=False)))
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
    lines = ["track scoring latency: %d launches per reading, %d readings, interleaved; ms per launch: median (lowest .. highest)" % (a.calls, a.reps)]
    for name, label, _, _ in variants:
        t = sorted(times[(name, label)])
        lines.append("%-34s %-50s %.4f (%.4f .. %.4f)" % (label, name, t[len(t) // 2], t[0], t[-1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
