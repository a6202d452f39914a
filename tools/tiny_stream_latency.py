"""Latency of a warm one-frame dt_tiny_stream_sequence against the stateless dt_tiny_sequence of the same shape.

    python tools/tiny_stream_latency.py --mode stream               # this tree: tiny_stream_sequence on warm slots
    python tools/tiny_stream_latency.py --mode stateless --root DIR # any tree (e.g. a checkout of the parent commit): tiny_sequence,
                                                                    # and the cost of ONE lstm_step launch from a profiled (n, 64) call

U = 512, D = 516, graphs on, shapes (n, T) = (1, 1), (64, 1), (512, 1), (32, 64).  Per shape: warm-up calls (the third call with a
shape replays its graph), then --repeats calls timed one by one with events on the stream; median, min and max are printed as one
JSON line per shape; c_call_* is the same call at the C entry with its arguments prepared once.  profiles/tiny_stream_latency.txt holds the numbers and the bar derived from them.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["stream", "stateless"], required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--shapes", default="1x1,64x1,512x1,32x64")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    import object_tracking_amd      # noqa: F401
    import mi355_dt
    from utility import synth

    torch.cuda.set_device(0)
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    n_max = max(n for n, _ in shapes)
    tw = synth.synth_tiny_weights(512)
    ctx = mi355_dt.Context()
    ctx.tiny_load(516, 512, tw["kernel"], tw["recurrent"], tw["bias"], tw["dense_kernel"], tw["dense_bias"])
    rows = torch.from_numpy(np.random.RandomState(7).rand(n_max, 64, 516).astype(np.float32)).to(ctx.device)
    if a.mode == "stream":
        ctx.tiny_stream_open(n_max)

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
        x = rows[:n, :T].contiguous()
        ctx.graph_enable(True)
        if a.mode == "stream":
            slots = list(range(n))
            ctx.tiny_stream_reset(slots)
            ctx.tiny_stream_sequence(x, slots)                      # the slots are warm from here on
            r = timed(lambda: ctx.tiny_stream_sequence(x, slots))
        else:
            r = timed(lambda: ctx.tiny_sequence(x))
        r.update(mode=a.mode, n=n, T=T)
        # the same call at the C entry, its arguments prepared once: what the Python wrapper (output tensor, slot list -> ctypes) adds
        out = torch.empty((n, T, 4), dtype=torch.float32, device=ctx.device)
        if a.mode == "stream":
            _, arr = ctx._slot_array(slots)
            c = timed(lambda: ctx.lib.dt_tiny_stream_sequence(ctx.h, x.data_ptr(), n, T, arr, out.data_ptr()))
        else:
            c = timed(lambda: ctx.lib.dt_tiny_sequence(ctx.h, x.data_ptr(), n, T, out.data_ptr()))
        r["c_call_median_ms"], r["c_call_min_ms"], r["c_call_max_ms"] = c["median_ms"], c["min_ms"], c["max_ms"]
        # one lstm_step launch at this n: a profiled (n, 64) call's lstm_step total over its launches (profiling bypasses the graphs).
        # In stream mode the call is the stream entry's, so the figure is the slot-addressed step's
        ctx.graph_enable(False)
        x64 = rows[:n].contiguous()
        call = (lambda: ctx.tiny_stream_sequence(x64, list(range(n)))) if a.mode == "stream" else (lambda: ctx.tiny_sequence(x64))
        call()
        ctx.profile_reset(); ctx.profile_enable(True)
        call()
        ctx.profile_enable(False)
        p = ctx.profile_read("lstm_step")
        r["step_ms"] = p["ms"] / max(1, p["launches"])
        r["step_launches"] = p["launches"]
        if a.mode == "stream":
            q = ctx.profile_read("stream_state")
            r["stream_state_ms"], r["stream_state_launches"] = q["ms"], q["launches"]
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
