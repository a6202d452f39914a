"""Latency of a warm track_stream call against the stateless track_clips call of the same shape.

    python tools/stream_latency.py --mode stream            # this tree: track_stream on warm slots
    python tools/stream_latency.py --mode clips --root DIR  # any tree (e.g. a checkout of the parent commit): track_clips,
                                                            # and the cost of ONE recurrent step from a profiled track_clips(n, 30)

416x416, graphs on, default policy, shapes (n, T) = (48, 30), (8, 1), (1, 1).  Per shape: warm-up calls (the third call with
a shape replays its graph), then --repeats calls timed one by one with events on the stream; median, min and max are
printed as one JSON line per shape.  profiles/stream_latency.txt holds the numbers and the bar derived from them.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["stream", "clips"], required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--shapes", default="48x30,8x1,1x1")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import object_tracking_amd      # noqa: F401
    import bench

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    n_max = max(n for n, _ in shapes)
    frames = bench.make_frames(n_max, 30, 416, 416, dev, seed0=42)
    trk, _, _ = bench.build_tracker(416, 416, 30, 32, frames[:min(n_max, 8)])
    ctx = trk.model.ctx
    if a.mode == "stream":
        trk.open_streams(n_max)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], repeats=len(ms))

    for n, T in shapes:
        x = frames[:n, :T].contiguous()
        ctx.graph_enable(True)
        if a.mode == "stream":
            slots = list(range(n))
            trk.reset_streams(slots)
            trk.track_stream(x, slots)                      # the slots are warm from here on
            r = timed(lambda: trk.track_stream(x, slots))
        else:
            r = timed(lambda: trk.track_clips(x))
        r.update(mode=a.mode, n=n, T=T, per_frame_ms=r["median_ms"] / T)
        if a.mode == "clips":       # one recurrent step at this n: the launches tagged convlstm_step of a profiled 30-frame call, over 29
            ctx.graph_enable(False)
            x30 = frames[:n].contiguous()
            trk.track_clips(x30)
            ctx.profile_reset(); ctx.profile_enable(True)
            trk.track_clips(x30)
            ctx.profile_enable(False)
            tags = [nm for nm in ctx.profile_names() if nm.endswith(":convlstm_step")]
            r["step_ms"] = sum(ctx.profile_read(nm)["ms"] for nm in tags) / 29.0
            r["step_tags"] = tags
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
