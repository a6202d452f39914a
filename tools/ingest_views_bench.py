#!/usr/bin/env python3
"""Frame views, measured: dt_ingest_views against dt_ingest_frames for 64 NV12 frames 1080x1920 -> 416x416.

    python tools/ingest_views_bench.py [--out profiles/ingest_views.txt] [--samples 25] [--calls 20]

Four cases in one run: dt_ingest_frames on the NV12 frames (the yardstick, re-measured here), dt_ingest_views on identity views of the same
frames (whole frame -> whole output: the same bytes), on letterboxed views ((0, 91, 416, 234): 44 % of the output rows are fill and read
nothing), and on a 960x540 crop of every frame, letterboxed.  The protocol is tools/ingest_frames_bench.py's: one process, no profiler,
both entries called through the C ABI with their arguments prepared beforehand; a sample is the HIP-event time of `calls` back-to-back
calls divided by `calls`; the cases take turns sample by sample; reported are the median of the samples and their spread (min .. max).
dt_ingest_views carries 32 views per launch, so 64 frames are two launches where dt_ingest_frames makes one.  Algorithmic bytes: the
source rectangle once (1.5 per NV12 pixel) plus the 3 * 416 * 416 bytes written per frame -- a figure of merit, not an HBM rate.
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
from utility.frames import FrameView, nv12_planes

DST = 416


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_views.txt"))
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    a = ap.parse_args()
    assert a.samples >= 20
    ctx = mi355_dt.Context()
    dev, lib, n = ctx.device, ctx.lib, a.frames
    ctx._sync_stream()
    hd = [torch.randint(0, 256, (1620, 1920), dtype=torch.uint8, device=dev) for _ in range(n)]
    items = [nv12_planes(s, 1080, 1920) for s in hd]
    out = torch.empty((n, DST, DST, 3), dtype=torch.uint8, device=dev)
    p_out = ctypes.c_void_p(out.data_ptr())
    d_frames = (mi355_dt.FrameDesc * n)(*[ctx._frame_desc(i, it, 0) for i, it in enumerate(items)])

    def views(descs):
        return (mi355_dt.FrameView * n)(*[ctx._frame_view(i, d, 0, DST, DST, "letterbox", (128, 128, 128)) for i, d in enumerate(descs)])

    v_ident = views([FrameView(it, fit="stretch") for it in items])
    v_lbox = views([FrameView(it) for it in items])
    v_crop = views([FrameView(it, crop=(480 + (i % 2), 270 + (i // 2) % 2, 960, 540)) for i, it in enumerate(items)])     # every parity of the origin
    assert (v_lbox[0].dst_x, v_lbox[0].dst_y, v_lbox[0].dst_w, v_lbox[0].dst_h) == (0, 91, 416, 234)
    w = 3.0 * DST * DST
    cases = [
        ("dt_ingest_frames  NV12 1080p", lambda: lib.dt_ingest_frames(ctx.h, d_frames, n, p_out, DST, DST), n * (1.5 * 1080 * 1920 + w)),
        ("dt_ingest_views   identity", lambda: lib.dt_ingest_views(ctx.h, v_ident, n, p_out, DST, DST), n * (1.5 * 1080 * 1920 + w)),
        ("dt_ingest_views   letterbox", lambda: lib.dt_ingest_views(ctx.h, v_lbox, n, p_out, DST, DST), n * (1.5 * 1080 * 1920 + w)),
        ("dt_ingest_views   960x540 crop, letterbox", lambda: lib.dt_ingest_views(ctx.h, v_crop, n, p_out, DST, DST), n * (1.5 * 540 * 960 + w)),
    ]
    # identity views give dt_ingest_frames' bytes
    assert cases[0][1]() == 0
    ref = out.clone()
    out.zero_()
    assert cases[1][1]() == 0
    assert torch.equal(out, ref), "dt_ingest_views on identity views differs from dt_ingest_frames"
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
    lines = ["# frame views, %d NV12 frames 1080x1920 -> %dx%d uint8; median of %d samples (each %d back-to-back calls, HIP events), spread = min .. max of the samples"
             % (n, DST, DST, a.samples, a.calls),
             "# device: %s" % torch.cuda.get_device_name(dev),
             "# launches per call: dt_ingest_frames %d (64 frames per launch), dt_ingest_views %d (32 views per launch)" % ((n + 63) // 64, (n + 31) // 32),
             "# %-42s %10s %22s %12s" % ("case", "median ms", "min .. max ms", "alg. GB/s")]
    med = []
    for (name, _, nbytes), ts in zip(cases, times):
        m = float(np.median(ts))
        med.append(m)
        lines.append("%-44s %10.4f %10.4f .. %-10.4f %10.1f" % (name, m, min(ts), max(ts), nbytes / (m * 1e-3) / 1e9))
    spread = max(times[0]) - min(times[0])
    verdict = "slower than" if med[1] - med[0] > spread else ("faster than" if med[0] - med[1] > spread else "within the spread of")
    lines.append("# dt_ingest_views on identity views is %s dt_ingest_frames: %+.4f ms against that entry's own spread of %.4f ms"
                 % (verdict, med[1] - med[0], spread))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
