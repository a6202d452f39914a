#!/usr/bin/env python3
"""Frame ingest, measured: dt_ingest_resize against dt_ingest_frames for 64 frames 1080x1920 -> 416x416.

    python tools/ingest_frames_bench.py [--out profiles/ingest_frames.txt] [--samples 25] [--calls 20]

Four cases: the existing entry on tight RGB24 frames (the yardstick, re-measured in this run), the new entry on the same RGB24 frames,
on NV12 frames, and on a mixed call of 32 x 1080p + 32 x 720p NV12 frames.  One process, no profiler.  Both entries are called through
the C ABI with their arguments prepared beforehand, so that the host work inside the timed window is the entry's own.  A sample is the
HIP-event time of `calls` back-to-back calls divided by `calls`; the cases take turns sample by sample, so that a disturbance of the
machine falls on all of them; reported are the median of the samples and their spread (min .. max).  Algorithmic bytes: every source
byte once (3 per RGB24 pixel, 1.5 per NV12 pixel) plus the 3 * 416 * 416 bytes written per frame -- as DESIGN.md 4.9 counts them; only
a fraction of the source is touched when downscaling 1080p, so the rate is a figure of merit, not an HBM rate.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import object_tracking_amd  # noqa: F401
import mi355_dt
from utility.frames import nv12_planes

DST = 416


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_frames.txt"))
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    a = ap.parse_args()
    assert a.samples >= 20
    ctx = mi355_dt.Context()
    dev, lib, n = ctx.device, ctx.lib, a.frames
    ctx._sync_stream()
    rgb = torch.randint(0, 256, (n, 1080, 1920, 3), dtype=torch.uint8, device=dev)
    hd = [torch.randint(0, 256, (1620, 1920), dtype=torch.uint8, device=dev) for _ in range(n)]
    sd = [torch.randint(0, 256, (1080, 1280), dtype=torch.uint8, device=dev) for _ in range(n // 2)]
    out = torch.empty((n, DST, DST, 3), dtype=torch.uint8, device=dev)
    p_out = ctypes.c_void_p(out.data_ptr())

    def descs(items):
        return (mi355_dt.FrameDesc * len(items))(*[ctx._frame_desc(i, it, 0) for i, it in enumerate(items)])

    d_rgb = descs([rgb[i] for i in range(n)])
    d_nv12 = descs([nv12_planes(s, 1080, 1920) for s in hd])
    mixed = [nv12_planes(hd[i // 2], 1080, 1920) if i % 2 == 0 else nv12_planes(sd[i // 2], 720, 1280) for i in range(n)]
    d_mixed = descs(mixed)
    p_rgb = ctypes.c_void_p(rgb.data_ptr())
    w = 3.0 * DST * DST
    cases = [
        ("dt_ingest_resize  RGB24 tight", lambda: lib.dt_ingest_resize(ctx.h, p_rgb, n, 1080, 1920, p_out, DST, DST), n * (3.0 * 1080 * 1920 + w)),
        ("dt_ingest_frames  RGB24 tight", lambda: lib.dt_ingest_frames(ctx.h, d_rgb, n, p_out, DST, DST), n * (3.0 * 1080 * 1920 + w)),
        ("dt_ingest_frames  NV12", lambda: lib.dt_ingest_frames(ctx.h, d_nv12, n, p_out, DST, DST), n * (1.5 * 1080 * 1920 + w)),
        ("dt_ingest_frames  NV12 1080p+720p", lambda: lib.dt_ingest_frames(ctx.h, d_mixed, n, p_out, DST, DST),
         (n // 2) * 1.5 * (1080 * 1920 + 720 * 1280) + n * w),
    ]
    # the two entries give the same bytes on the frames both take
    assert cases[0][1]() == 0
    ref = out.clone()
    out.zero_()
    assert cases[1][1]() == 0
    assert torch.equal(out, ref), "dt_ingest_frames differs from dt_ingest_resize on tight RGB24 frames"
    for _, fn, _ in cases:          # warm-up: every case, several calls
        for _ in range(5):
            assert fn() == 0
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(a.samples):
        for k, (_, fn, _) in enumerate(cases):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.calls)
    lines = ["# frame ingest, %d frames -> %dx%d uint8; median of %d samples (each %d back-to-back calls, HIP events), spread = min .. max of the samples"
             % (n, DST, DST, a.samples, a.calls),
             "# device: %s" % torch.cuda.get_device_name(dev),
             "# %-36s %10s %22s %12s" % ("case", "median ms", "min .. max ms", "alg. GB/s")]
    med = []
    for (name, _, nbytes), ts in zip(cases, times):
        m = float(np.median(ts))
        med.append(m)
        lines.append("%-38s %10.4f %10.4f .. %-10.4f %10.1f" % (name, m, min(ts), max(ts), nbytes / (m * 1e-3) / 1e9))
    spread = max(times[0]) - min(times[0])
    verdict = "slower than" if med[1] - med[0] > spread else ("faster than" if med[0] - med[1] > spread else "within the spread of")
    lines.append("# dt_ingest_frames on tight RGB24 is %s dt_ingest_resize: %+.4f ms against that entry's own spread of %.4f ms"
                 % (verdict, med[1] - med[0], spread))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
