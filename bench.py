#!/usr/bin/env python3
"""bench.py -- frames/s of the detect-and-track hot path on MI355X.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python bench.py --gpus N --steps K --warmup W        # N > 1 without a launcher: re-executes itself under
                                                         # torch.distributed.run, one rank per GPU (RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Workload (default `--workload track`, BASELINE.json configs[2], the 1-GPU
configuration the metric "frames/sec detect+track @416x416" is quoted on):
per GPU `--clips` MOT17-shaped synthetic clips of T=30 frames, 416x416x3 uint8,
already resident in HBM; one STEP = one pass of the whole path over that batch:
  x/255 + YOLOv2 (23 conv, C=12)  ->  ConvLSTM2D(512,3x3) recurrence over T
  -> 1x1 conv -> decode_netout + NMS for every frame -> track-id association
  (+ for N>1 the cross-stream all-gather of the detection records).
`--workload detect` runs BASELINE.json configs[1] instead (YOLOv2 C=80 forward
+ decode, batch 8) -- reported as an extra line item, never as `value`.

Synthetic data: darknet-format random weights (utility/synth.py, seeds
1234/1235); the tracker's 1x1 head is calibrated once, outside the timed region,
so that ~32 boxes/frame survive (the "32 tracks" of configs[2]); frames are
low-frequency backgrounds with moving rectangles.

A plain run sets up, warms up, times --steps steps and prints ONE JSON line on rank 0: metric, value (frames/s), unit,
higher_is_better, dtype, ms_per_step (one timed step), the configuration and, for N > 1, the per-rank figures.
  --dump-outputs DIR  after the timed steps, writes what the LAST timed step computed -- the arrays a caller of the
                      step receives (track: boxes, counts, ids, nids, netout) -- as DIR/<name>.npy, float32 (float
                      results) or float64 (integer results); an array over its share of 64 MB is replaced by a fixed
                      seeded sample of its flattened elements (the same elements for the same arguments).
  --full              everything else, behind the headline steps (off by default): the instrumented per-kernel pass
                      (kernels, roofline, --layer-report) and, at --gpus 1 for the track workload, the extra
                      configurations (--no-extra) and the CPU baseline (--no-cpu-baseline).
With --full the line also holds
  roofline     -- achieved / peak / frac / traffic of the DOMINANT kernel family (the one with the most HIP-event
                  time inside the timed region; with the default policy wino_gemm_s3_kernel: executed fp16 MFMA
                  FLOPs -- three per fp32 multiply-add of two-term split operands -- against the 2.5 PFLOP/s dense
                  16-bit peak of MI355X), and under roofline.families one self-contained block per conv kernel family
                  (wino_gemm_s3 / conv3_h2 / conv_igemm_f32 against the 157.3 TFLOP/s fp32 matrix peak / wino4s_fused /
                  conv1_mfma): launches, time, executed and
                  direct-form FLOPs of the layers THOSE launches computed, bytes, PMC traffic
  cpu_baseline -- the CPU oracle ("port") timed on a bounded sample on this host.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

import object_tracking_amd  # noqa: F401
from models_detection.KerasYOLO import KerasYOLO
from models_tracking.MultiObjDetTracker import MultiObjDetTracker
from parallel import frame_shard_stage_ms, gather_detections, init_from_env, track_clips_frame_sharded
from utility import synth

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU x 2.4 GHz
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16 dense (16x the fp32 MFMA rate)
PEAK_HBM_GBS = 8000.0
GFLOP_TRACK_416 = 39.460          # 29.346 detect (C=12) + 10.099 ConvLSTM + 0.015 1x1
GFLOP_DETECT_416_C80 = 29.464


def make_frames(n_clips, T, H, W, device, seed0):
    """uint8 [n_clips,T,H,W,3] on the device.  Up to 8 distinct clips are rendered
    on the host (utility/synth.synth_clip); further clips are spatial rolls of them."""
    base = [torch.from_numpy(synth.synth_clip(T, H, W, 32, seed=seed0 + i)) for i in range(min(n_clips, 8))]
    out = torch.empty((n_clips, T, H, W, 3), dtype=torch.uint8, device=device)
    for i in range(n_clips):
        src = base[i % len(base)].to(device)
        if i >= len(base):
            src = torch.roll(src, shifts=(17 * (i // len(base)), 29 * (i // len(base))), dims=(1, 2))
        out[i] = src
    return out


def build_tracker(H, W, T, target_boxes, frames_for_calib):
    class Trk(MultiObjDetTracker):
        IMAGE_H, IMAGE_W = H, W
        GRID_H, GRID_W = H // 32, W // 32
        SEQUENCE_LENGTH = T
        LOAD_MODEL = False

    C = len(Trk.LABELS)
    blob = synth.synth_darknet_blob(C, seed=1234)
    tw = synth.synth_tracker_weights(C, seed=1235)
    S = 5 + C
    cls_ch = [b * S + 5 + c for b in range(5) for c in range(C)]
    obj_ch = [b * S + 4 for b in range(5)]
    tw["out_kernel"][..., cls_ch] *= 200.0          # peaky class softmax: score ~ objectness
    tw["out_bias"][obj_ch] = 0.0
    trk = Trk(detector_weights=blob, tracker_weights=tw)
    # calibration (untimed): shift the objectness bias so that ~target_boxes cells/frame have t_o > 0
    netout = trk.model.forward(frames_for_calib, want_det=False)
    to = netout[..., 4].reshape(netout.shape[0] * netout.shape[1], -1).float()
    k = max(1, min(to.shape[1] - 1, to.shape[1] - target_boxes))
    q = torch.kthvalue(to, k, dim=1).values.mean().item()
    tw["out_bias"][obj_ch] = -q
    trk.model.set_weights(tw)
    return trk, blob, tw


def cpu_baseline_track(blob, tw, H, W, n_frames):
    """The CPU statements of the path ("port" of the Keras graph, not Keras itself -- SURVEY.md section 0.1) on a
    bounded sample: one clip of n_frames frames through detector, ConvLSTM, 1x1, decode and association.  Two
    variants are timed -- oracle/oracle.c (C + OpenMP loop nest) and oracle/torch_cpu.py (ATen/oneDNN convolutions) --
    each warmed up and with the thread count that is fastest on this host (a short sweep on the detector: the GPU
    boxes' 256 logical cores are slower with every thread busy than with 32), and the FASTER one is the reported
    baseline.  Returns {variant: (frames/s, seconds, threads)}."""
    from oracle import oracle as orc
    from oracle import torch_cpu
    C = 12
    layers, _ = orc.parse_darknet_blob(blob, C)
    frames = orc.normalize_u8(synth.synth_clip(n_frames, H, W, 32, seed=999))
    ncpu = os.cpu_count() or 1
    try:
        aff0 = set(os.sched_getaffinity(0))              # the cores this process may run on (cgroup / taskset), not the host's count
    except (AttributeError, OSError):
        aff0 = set(range(ncpu))
    # ONE NUMA node: frame-at-a-time convolutions spread over two sockets got SLOWER beyond 16-32 threads in round 5 (remote memory, no
    # binding).  Every thread of this process is bound to the cores of the node with the most usable cores for the CPU leg and released after.
    node_cpus, bound = _numa_node_cpus(aff0), None
    if node_cpus and len(node_cpus) < len(aff0):
        bound = _bind_all_threads(node_cpus)
    naff = len(node_cpus) if bound is not None else len(aff0)
    nphys = _physical_cores(node_cpus if bound is not None else aff0)
    cand = sorted({n for n in (naff, nphys, nphys // 2, naff // 2, 64, 32, 16, 8) if 1 <= n <= naff} or {1}, reverse=True)
    sample = frames[:min(8, n_frames)]
    sweeps = {}

    def sweep(tag, set_threads, fwd):
        """every candidate thread count on an 8-frame detector pass, no early exit; the fastest is used for the timed clip"""
        best = (None, 1e30)
        sweeps[tag] = {}
        for nt in cand:
            set_threads(nt)
            fwd(sample[:1], layers)                      # primitive creation / page-in outside the timed pass
            t0 = time.perf_counter()
            fwd(sample, layers)
            dt = time.perf_counter() - t0
            sweeps[tag][nt] = len(sample) / dt
            if dt < best[1]:
                best = (nt, dt)
        set_threads(best[0])
        return best[0]

    out = {}
    default_torch = torch.get_num_threads()
    def torch_variant(cl):
        def with_layout(f):
            def g(*a):
                torch_cpu.CHANNELS_LAST = cl
                return f(*a)
            return g
        return with_layout(torch_cpu.tracker_forward), with_layout(torch_cpu.yolov2_forward)

    for name, fwd, det_fwd, set_threads in (
            ("oracle_c_openmp", orc.tracker_forward, orc.yolov2_forward, orc.set_threads),
            ("torch_cpu_onednn_nhwc",) + torch_variant(True) + (torch.set_num_threads,),
            ("torch_cpu_onednn_nchw",) + torch_variant(False) + (torch.set_num_threads,)):
        nt = sweep(name, set_threads, det_fwd)
        t0 = time.perf_counter()
        trk, _ = fwd(frames, layers, tw)
        cap = trk.shape[1] * trk.shape[2] * 5
        rb = np.zeros((n_frames, cap, 8), dtype=np.float32)
        rc = np.zeros(n_frames, dtype=np.int32)
        for t in range(n_frames):
            rows, _ = orc.decode_netout(trk[t], 0.5, 0.45, MultiObjDetTracker.ANCHORS, C)
            rb[t, :len(rows)] = rows
            rc[t] = len(rows)
        orc.associate_clip(rb, rc, 0.3)
        dt = time.perf_counter() - t0
        out[name] = (n_frames / dt, dt, nt)
    torch.set_num_threads(default_torch)
    orc.set_threads(len(aff0))
    if bound is not None:
        _bind_all_threads(aff0)
    out["_host"] = {"host_logical_cores": ncpu, "affinity_cores": len(aff0), "numa_node_cores_bound": naff if bound is not None else None,
                    "physical_cores_in_binding": nphys, "detector_frames_per_s_by_threads": sweeps}
    return out


def _parse_cpulist(txt):
    cpus = set()
    for part in txt.strip().split(","):
        if not part:
            continue
        a, _, b = part.partition("-")
        cpus.update(range(int(a), int(b or a) + 1))
    return cpus


def _numa_node_cpus(allowed):
    """usable cpus of the NUMA node that has the most of them (None if the host does not say)"""
    import glob
    best = None
    for d in glob.glob("/sys/devices/system/node/node[0-9]*"):
        try:
            cpus = _parse_cpulist(open(os.path.join(d, "cpulist")).read()) & set(allowed)
        except (OSError, ValueError):
            continue
        if cpus and (best is None or len(cpus) > len(best)):
            best = cpus
    return best


def _physical_cores(cpus):
    seen = set()
    for c in cpus:
        try:
            seen.add(min(_parse_cpulist(open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % c).read())))
        except (OSError, ValueError):
            seen.add(c)
    return max(1, len(seen))


def _bind_all_threads(cpus):
    """affinity of every thread this process has (OpenMP / ATen pools keep the mask they were created with otherwise)"""
    n = 0
    for tid in os.listdir("/proc/self/task"):
        try:
            os.sched_setaffinity(int(tid), cpus)
            n += 1
        except (OSError, ValueError):
            pass
    return n


def detect_batch8_extra(device, H, W, seed0):
    """BASELINE.json configs[1] under the same clock: YOLOv2 C=80 forward + decode/NMS on 8 frames, plain launches
    and hipGraph replay, in its own context, after the main timed region."""
    C, B = 80, 8
    blob = synth.synth_darknet_blob(C, seed=1234)
    det = KerasYOLO({'LABELS': KerasYOLO.LABELS_COCO, 'BATCH_SIZE': B, 'IMAGE_H': H, 'IMAGE_W': W,
                     'GRID_H': H // 32, 'GRID_W': W // 32}, weights=blob)
    frames = make_frames(1, B, H, W, device, seed0=seed0)[0].contiguous()
    out = {"workload": "BASELINE.json configs[1]: YOLOv2 C=80 forward + decode/NMS, batch 8, %dx%d uint8" % (H, W)}
    for label, graphs in (("plain", False), ("graphs", True)):
        det.model.ctx.graph_enable(graphs)
        for _ in range(5):
            det.detect(frames)
        torch.cuda.synchronize()
        n = 50
        t0 = time.perf_counter()
        for _ in range(n):
            det.detect(frames)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / n
        out[label] = {"ms_per_batch": ms, "frames_per_s": B / (ms * 1e-3),
                      "direct_form_tflops": B * GFLOP_DETECT_416_C80 * (H * W) / (416.0 * 416.0) / ms}
    det.model.ctx.graph_enable(False)
    # roofline-style block of this configuration: an instrumented pass (HIP events per launch), the bytes of weights a forward streams by the
    # library's own count (at batch 8 the 13x13 layers are bound by them: Winograd-domain weights are 64 / 9 (F(6x6)) or 36 / 9 (F(4x4)) times
    # the direct form's), and what those bytes cost at the 5 TB/s a streaming kernel reaches
    ctx = det.model.ctx
    ctx.profile_reset(); ctx.profile_enable(True)
    n = 10
    for _ in range(n):
        det.detect(frames)
    ctx.profile_enable(False)
    fam = {}
    for name in ("conv_gemm_s3", "conv_igemm", "conv_direct_h2", "conv_fused", "wino_input", "wino_output", "conv1_direct", "splitk_reduce", "decode_nms", "absmax"):
        pr = ctx.profile_read(name)
        if pr["launches"]:
            fam[name] = {"launches_per_forward": pr["launches"] / n, "ms_per_forward": pr["ms"] / n,
                         "executed_tflops": (pr["flops"] / (pr["ms"] * 1e-3) / 1e12) if pr["ms"] > 0 else None,
                         "implementation_GBps": (pr["bytes"] / (pr["ms"] * 1e-3) / 1e9) if pr["ms"] > 0 else None}
    wbytes = 0.0
    layers = {}
    for name in ctx.profile_names():
        if name.startswith("conv_igemm:") or name.startswith("conv_gemm_s3:"):
            pr = ctx.profile_read(name)
            if pr["ms"] > 0:
                layers[name] = {"ms_per_forward": pr["ms"] / n, "executed_tflops": pr["flops"] / (pr["ms"] * 1e-3) / 1e12,
                                "implementation_MB_per_forward": pr["bytes"] / n / 1e6}
                wbytes += pr["bytes"] / n
    direct_w = 203.8e6
    kernel_ms = sum(v["ms_per_forward"] for v in fam.values())
    out["roofline"] = {"bound": "hbm (weights) at this batch: 23 layers, %d launches, no layer has more than 8 x 43264 rows" % int(sum(v["launches_per_forward"] for v in fam.values())),
                       "kernel_ms_per_forward": kernel_ms, "families": fam,
                       "gemm_operand_bytes_per_forward": wbytes, "direct_form_weight_bytes": direct_w,
                       "hbm_ms_of_gemm_operand_bytes_at_5TBps": wbytes / 5e12 * 1e3,
                       "hbm_ms_of_direct_form_weights_at_5TBps": direct_w / 5e12 * 1e3,
                       "direct_form_tflops_over_kernel_time": B * GFLOP_DETECT_416_C80 * (H * W) / (416.0 * 416.0) / kernel_ms if kernel_ms > 0 else None,
                       "gemm_layers": layers,
                       "note": "instrumented pass (plain launches, an event pair per launch); gemm_operand_bytes = V + U + M' of every GEMM launch by the library's own "
                               "count -- dominated by the Winograd-domain weights U of the 13x13 layers; the gap between kernel_ms and ms_per_batch is launch latency"}
    return out


DUMP_BYTES = 60 * 10 ** 6       # under 64 MB with the .npy headers


def dump_outputs(dirname, res):
    """--dump-outputs: every tensor of a step's result as <dirname>/<name>.npy -- float32 for float results, float64 for
    integer ones (exact) -- within DUMP_BYTES in all: an array over its equal share is replaced by a fixed seeded sample
    of its flattened elements, in index order."""
    if torch.is_tensor(res):
        items = [("output", res)]
    elif isinstance(res, dict):
        items = [(k, v) for k, v in sorted(res.items()) if torch.is_tensor(v)]
    else:
        items = [("output%d" % i, v) for i, v in enumerate(res) if torch.is_tensor(v)]
    os.makedirs(dirname, exist_ok=True)
    for name, t in items:
        dtype, size = (torch.float32, 4) if t.is_floating_point() else (torch.float64, 8)
        cap = DUMP_BYTES // len(items) // size
        flat = t.detach().reshape(-1)
        if flat.numel() > cap:
            idx = np.sort(np.random.default_rng(0).choice(flat.numel(), cap, replace=False))
            arr = flat[torch.from_numpy(idx).to(flat.device)].to(dtype).cpu().numpy()
        else:
            arr = t.detach().to(dtype).cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), arr)


def _time_steps(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def track_extra(device, size, clips, T, boxes, steps=3, env=None, what=None, graphs=False, want_det=False):
    """BASELINE.json configs[4]'s single-GPU shard under the same clock: MultiObjDetTracker at size x size with
    ~`boxes` candidate boxes per frame, `clips` clips x T frames per step, its own context.  `env`: policy knobs the
    context is created under (read once in dt_create), e.g. {"DT_S3": "0"} = every GEMM on the fp32 MFMA instruction."""
    frames = make_frames(clips, T, size, size, device, seed0=7000)
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        trk, _, _ = build_tracker(size, size, T, boxes, frames)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    cap = max(128, 2 * boxes)
    res = {}
    if graphs:
        trk.model.ctx.graph_enable(True)      # captured on the second warm-up call, replayed afterwards

    def step():
        if want_det:
            grids = trk.model.forward(frames, want_det=True)
            res["r"] = trk.decode_and_associate(grids[0] if isinstance(grids, (tuple, list)) else grids, cap=cap)
        else:
            res["r"] = trk.track_clips(frames, cap=cap)
    sec = _time_steps(step, 3 if graphs else 2, steps)
    return {"workload": what or "BASELINE.json configs[4] on one GPU: MultiObjDetTracker %dx%d, %d clips x %d frames per step, "
                                "head calibrated to %d candidate boxes per frame" % (size, size, clips, T, boxes),
            "ms_per_step": 1e3 * sec, "frames_per_s": clips * T / sec,
            "boxes_per_frame": float(res["r"]["counts"].float().mean().item())}


def tiny_extra(device, H, W, seqs, steps=3):
    """BASELINE.json configs[3] on one GPU under the same clock: TinyTracker over `seqs` sequences x 64 frames
    (YOLOv2 C=80 + act_13 global max-pool + decode / top box per frame, LSTM(512) + Dense(4) over T)."""
    from models_tracking.TinyTracker import TinyTracker
    C, T = 80, 64
    blob = synth.synth_darknet_blob(C, seed=1234)
    det = KerasYOLO({'LABELS': KerasYOLO.LABELS_COCO, 'BATCH_SIZE': 4, 'IMAGE_H': H, 'IMAGE_W': W,
                     'GRID_H': H // 32, 'GRID_W': W // 32}, weights=blob)
    ctx = det.model.ctx
    cfg = {"model_tracker": {"name": "TinyTracker", "lstm_units": 512, "sequence_length": T},
           "train": {"pool": "Global", "batch_size": 4}}
    tt = TinyTracker(cfg, feature_dims=(H // 16, W // 16, 512), weights=synth.synth_tiny_weights(512), ctx=ctx)
    frames = make_frames(seqs, T, H, W, device, seed0=9000)

    def step():
        rows, _ = tt.frame_rows(frames.reshape(seqs * T, H, W, 3), det)
        return ctx.tiny_sequence(rows.reshape(seqs, T, -1).contiguous())
    sec = _time_steps(step, 2, steps)
    return {"workload": "BASELINE.json configs[3] on one GPU: TinyTracker, %d sequences x %d frames, %dx%d" % (seqs, T, H, W),
            "ms_per_step": 1e3 * sec, "frames_per_s": seqs * T / sec}


def load_traffic(clips, T, size):
    """PMC-derived bytes per launch of the dominant GEMM kernel for this exact workload, measured
    with rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over
    tools/pmc_probe.py and committed under profiles/ (tools/make_traffic_json.py).
    bench.py cannot collect hardware counters itself; returns None if no
    committed measurement matches the workload."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*traffic*.json"))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        w = d.get("workload", {})
        if (w.get("clips"), w.get("T"), w.get("size")) == (clips, T, size):
            best = (f, d)
    return best


def instrumented_report(args, ctx, step, sync_all, rank):
    """--full: the per-kernel table and the roofline, from a pass of their own behind the timed steps.  Returns the fields of
    the JSON line that come from it."""
    # ---- a SEPARATE instrumented pass for the per-kernel table and the roofline: HIP events around every launch, on the launch
    # stream (with --graphs: none -- profiling bypasses the replayed graphs, so the table then describes plain launches) ----
    prof_steps = max(1, min(args.prof_steps, args.steps))
    if args.graphs:
        ctx.graph_enable(False)       # per-launch events need plain launches
    ctx.profile_reset()
    ctx.profile_enable(True)
    sync_all()
    t1 = time.perf_counter()
    for _ in range(prof_steps):
        step()
    sync_all()
    elapsed_prof = time.perf_counter() - t1
    ctx.profile_enable(False)

    kern = {}
    for name in ("conv_gemm_s3", "conv_igemm", "conv_direct_h2", "conv_fused", "wino_input", "wino_output", "conv1_direct", "convlstm_gates", "decode_nms", "associate", "splitk_reduce", "pool",
                 "lstm_step", "misc"):
        p = ctx.profile_read(name)
        if p["launches"]:
            kern[name] = dict(launches=p["launches"], ms_per_step=p["ms"] / prof_steps,
                              tflops=(p["flops"] / (p["ms"] * 1e-3) / 1e12) if p["ms"] > 0 else None,
                              gbs=(p["bytes"] / (p["ms"] * 1e-3) / 1e9) if p["ms"] > 0 else None)
    steps = prof_steps               # every per-kernel figure below comes from the instrumented pass
    ig = ctx.profile_read("conv_igemm")
    s3 = ctx.profile_read("conv_gemm_s3")
    fused = ctx.profile_read("conv_fused")
    c3h2 = ctx.profile_read("conv_direct_h2")
    conv1 = ctx.profile_read("conv1_direct")
    wino_in, wino_out = ctx.profile_read("wino_input"), ctx.profile_read("wino_output")
    wino_ms = wino_in["ms"] + wino_out["ms"]
    # direct-form work (2*M*K*N of the reference's layer; in + W + out fp32 bytes) of the layers EACH family's
    # launches computed -- booked per family by the library (network.hip:prof_direct_form), never across families
    df = {"conv_gemm_s3": ctx.profile_read("conv_direct_form_s3"), "conv_igemm": ctx.profile_read("conv_direct_form"),
          "conv_fused": ctx.profile_read("conv_direct_form_fused"), "conv_direct_h2": ctx.profile_read("conv_direct_form_c3h2"),
          "conv1_direct": ctx.profile_read("conv_direct_form_conv1")}
    conv1_bf16 = ctx.profile_read("conv1_direct:bf16")["launches"] > 0      # conv1_s3_kernel (default) or the fp32 MFMA kernel (DT_S3_CONV1=0 / DT_S3=0)
    tr = load_traffic(args.clips, args.T, args.size) if args.workload == "track" else None
    fam_traffic = (tr[1].get("family_bytes_per_step") or {}) if tr is not None else {}

    def family(key, prof, kernel, instruction, peak, tkey):
        """one kernel family: everything from ITS launches, ITS HIP-event time and ITS PMC bytes"""
        if prof["ms"] <= 0:
            return None
        sec, n = prof["ms"] * 1e-3, max(1, prof["launches"])
        d = {"kernel": kernel, "instruction": instruction, "peak_tflops": peak,
             "launches_per_step": prof["launches"] / steps, "ms_per_step": prof["ms"] / steps, "avg_launch_ms": prof["ms"] / n,
             "executed_tflop_per_step": prof["flops"] / steps / 1e12, "executed_gflop_per_launch": prof["flops"] / n / 1e9,
             "achieved": prof["flops"] / sec / 1e12, "frac": prof["flops"] / sec / 1e12 / peak,
             "algorithmic_tflop_per_step": df[key]["flops"] / steps / 1e12, "algorithmic_gflop_per_launch": df[key]["flops"] / n / 1e9,
             "achieved_algorithmic": df[key]["flops"] / sec / 1e12,
             "direct_form_bytes_per_step": df[key]["bytes"] / steps,
             "implementation_bytes_per_launch": prof["bytes"] / n, "implementation_GBps": prof["bytes"] / sec / 1e9,
             "traffic_bytes_per_launch": None, "traffic_bytes_per_step": None}
        if tkey in fam_traffic:
            d["traffic_bytes_per_step"] = fam_traffic[tkey]
            d["traffic_bytes_per_launch"] = fam_traffic[tkey] / (prof["launches"] / steps)
        return d

    # which operand form the split GEMMs ran in (the library counts its launches per form): fp16 x 2 terms / three products (default since
    # round 6) or bf16 x 3 terms / six products (DT_S3_H2=0, DT_PIN)
    n_h2, n_b3 = ctx.profile_read("s3_form:f16x2")["launches"], ctx.profile_read("s3_form:bf16x3")["launches"]
    s3_h2 = n_h2 > 0 and n_b3 == 0
    s3_products = 3.0 if s3_h2 else 6.0
    families = {
        "wino_gemm_s3": family("conv_gemm_s3", s3, "wino_gemm_s3_kernel / wino_gemm_s3_half_kernel (F(6x6) / F(4x4) batched GEMMs, 1x1 layers behind them)",
                               ("v_mfma_f32_32x32x16_f16 on 2-term split fp32 operands scaled into fp16's range (hi + lo, 22+ bits), three per fp32 "
                                "multiply-add, fp32 accumulate" if s3_h2 else
                                "v_mfma_f32_32x32x16_bf16 on 3-term split fp32 operands, six per fp32 multiply-add, fp32 accumulate"),
                               PEAK_BF16_MFMA_TFLOPS, "wino_gemm_s3"),
        "conv_igemm_f32": family("conv_igemm", ig, "conv_igemm_f32 (implicit GEMM: the 1x1 layers with fewer than 128 output channels -- conv_4, conv_21, conv_23, tconv_2)",
                                 "v_mfma_f32_32x32x2_f32", PEAK_F32_MFMA_TFLOPS, "conv_igemm_f32"),
        "conv3_h2": family("conv_direct_h2", c3h2, "conv3_h2_kernel (conv_2 / conv_3 / conv_5: direct 3x3 convolution, patch resident in LDS, + BN + LeakyReLU [+ 2x2 max])",
                           "v_mfma_f32_32x32x16_f16 on 2-term split fp32 operands scaled into fp16's range, three per fp32 multiply-add, fp32 accumulate",
                           PEAK_BF16_MFMA_TFLOPS, "conv3_h2"),
        "wino4s_fused": family("conv_fused", fused, "wino4s_fused_kernel (conv_2 / conv_3 / conv_5: fused F(4x4,3x3))", "v_mfma_f32_16x16x4_f32",
                               PEAK_F32_MFMA_TFLOPS, "wino4s_fused"),
        "conv1_mfma": family("conv1_direct", conv1, "conv1_s3_kernel (conv_1 + x/255 + BN + LeakyReLU + 2x2 max; K = 27 padded to 32)" if conv1_bf16 else
                             "conv1_mfma_kernel (conv_1 + x/255 + BN + LeakyReLU + 2x2 max; K = 27 padded to 28)",
                             "v_mfma_f32_32x32x16_bf16: uint8 values are exact bf16 numbers, weights / 255 as three bf16 terms, three per multiply-add" if conv1_bf16
                             else "v_mfma_f32_32x32x2_f32", PEAK_BF16_MFMA_TFLOPS if conv1_bf16 else PEAK_F32_MFMA_TFLOPS, "conv1_mfma"),
    }
    if families["wino_gemm_s3"]:
        families["wino_gemm_s3"]["operand_form"] = "f16x2" if s3_h2 else ("bf16x3" if n_h2 == 0 else "mixed")
        families["wino_gemm_s3"]["mfma_products_per_multiply"] = s3_products
        families["wino_gemm_s3"]["fp32_equivalent_tflops"] = families["wino_gemm_s3"]["achieved"] / s3_products
        families["wino_gemm_s3"]["fp32_equivalent_over_fp32_mfma_peak"] = families["wino_gemm_s3"]["achieved"] / s3_products / PEAK_F32_MFMA_TFLOPS
    transforms = None if wino_ms <= 0 else {
        "kernel": "wino_input_* / wino_output_* (Winograd transforms around the batched GEMMs)", "bound": "hbm", "peak_GBps": PEAK_HBM_GBS,
        "launches_per_step": (wino_in["launches"] + wino_out["launches"]) / steps, "ms_per_step": wino_ms / steps,
        "input_ms_per_step": wino_in["ms"] / steps, "output_ms_per_step": wino_out["ms"] / steps,
        "implementation_GBps": (wino_in["bytes"] + wino_out["bytes"]) / (wino_ms * 1e-3) / 1e9,
        "frac_of_8TBps": (wino_in["bytes"] + wino_out["bytes"]) / (wino_ms * 1e-3) / 8e12,
        "implementation_bytes_per_step": (wino_in["bytes"] + wino_out["bytes"]) / steps,
        "traffic_bytes_per_step": fam_traffic.get("wino_transforms"),
        "input_GBps": (wino_in["bytes"] / (wino_in["ms"] * 1e-3) / 1e9) if wino_in["ms"] > 0 else None,
        "output_GBps": (wino_out["bytes"] / (wino_out["ms"] * 1e-3) / 1e9) if wino_out["ms"] > 0 else None,
        # what a plain streaming kernel reaches on an MI355X of this pool, per traffic mix (tools/micro/hbm_rw, profiles/r04_hbm_ceilings.txt):
        # the split input transforms write 2.7 bytes per byte read, the output transforms read 1.8 per byte written
        "streaming_kernel_GBps": {"read_only": 5670, "write_only": 4400, "copy": 4800, "1_read_to_2.7_writes": 4250, "1.8_reads_to_1_write": 4850,
                                  "note": "means over three boxes; +/- 5 % between boxes; ONE launch geometry (grid 4096 x 256, 16 B per lane, nontemporal)",
                                  "source": "profiles/r04_hbm_ceilings.txt"},
        # the best of a sweep over grid / block / unroll / cache policy per mix (tools/probes/hbm_sweep.hip, profiles/r06_experiments.txt section 9):
        # a plain stream's rate moves +/- 25 % with the launch geometry
        "streaming_kernel_best_geometry_GBps": {"read_only": 7200, "write_only": 6300, "copy": 6000, "1_read_to_2.7_writes": 4800, "1.8_reads_to_1_write": 5400,
                                                "source": "profiles/r06_hbm_sweep.txt (one box)"}}
    dominant = max((k for k in families if families[k]), key=lambda k: families[k]["ms_per_step"], default=None)
    # whole conv path: time the matrix pipe would need AT ITS PEAKS for everything the conv kernels execute (bf16 and fp32
    # instructions have different peaks) / the time the conv path takes, transforms included
    conv_path_ms = s3["ms"] + ig["ms"] + fused["ms"] + c3h2["ms"] + conv1["ms"] + wino_ms
    conv_path_flops = ig["flops"] + fused["flops"] + (0.0 if conv1_bf16 else conv1["flops"])      # executed on the fp32 MFMA instructions
    conv_path_bf16 = s3["flops"] + c3h2["flops"] + (conv1["flops"] if conv1_bf16 else 0.0)           # ... on the 16-bit instructions
    conv_path_pipe_frac = ((conv_path_bf16 / (PEAK_BF16_MFMA_TFLOPS * 1e12) + conv_path_flops / (PEAK_F32_MFMA_TFLOPS * 1e12)) /
                           (conv_path_ms * 1e-3)) if conv_path_ms > 0 else None
    direct_form_all = sum(v["flops"] for v in df.values())
    direct_form_bytes_all = sum(v["bytes"] for v in df.values())
    # conv_igemm_f32's launches by arithmetic intensity (executed FLOP per algorithmic byte): below the ridge of the chip
    # (157.3 TFLOP/s over ~6.3 TB/s achievable = 25 FLOP/B; 40 used as the class boundary) a launch is HBM-bound whatever
    # the kernel does, and is priced against the HBM roof instead
    regimes = {"mfma": [0.0, 0.0, 0.0, []], "hbm": [0.0, 0.0, 0.0, []]}
    for name in ctx.profile_names():
        if not name.startswith("conv_igemm:"):
            continue
        p = ctx.profile_read(name)
        if p["ms"] <= 0 or p["bytes"] <= 0:
            continue
        r = regimes["mfma" if p["flops"] / p["bytes"] >= 40.0 else "hbm"]
        r[0] += p["flops"]; r[1] += p["bytes"]; r[2] += p["ms"]; r[3].append(name.split(":", 1)[1])
    if families["conv_igemm_f32"]:
        families["conv_igemm_f32"]["mfma_bound_launches"] = None if regimes["mfma"][2] <= 0 else {
            "layers": sorted(regimes["mfma"][3]), "ms_per_step": regimes["mfma"][2] / steps,
            "achieved": regimes["mfma"][0] / (regimes["mfma"][2] * 1e-3) / 1e12,
            "frac": regimes["mfma"][0] / (regimes["mfma"][2] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS}
        families["conv_igemm_f32"]["hbm_bound_launches"] = None if regimes["hbm"][2] <= 0 else {
            "layers": sorted(regimes["hbm"][3]), "ms_per_step": regimes["hbm"][2] / steps,
            "achieved_GBps": regimes["hbm"][1] / (regimes["hbm"][2] * 1e-3) / 1e9,
            "frac_of_8TBps": regimes["hbm"][1] / (regimes["hbm"][2] * 1e-3) / 8e12,
            "executed_tflops": regimes["hbm"][0] / (regimes["hbm"][2] * 1e-3) / 1e12}
    for key, fam in (("conv_gemm_s3:", "wino_gemm_s3"), ("conv_igemm:", "conv_igemm_f32"), ("conv_fused:", "wino4s_fused"), ("conv_direct_h2:", "conv3_h2")):
        if not families[fam]:
            continue
        layers = {}
        for name in ctx.profile_names():
            if name.startswith(key):
                p = ctx.profile_read(name)
                if p["ms"] > 0:
                    layers[name.split(":", 1)[1]] = {"ms_per_step": p["ms"] / steps, "launches_per_step": p["launches"] / steps,
                                                    "executed_tflops": p["flops"] / (p["ms"] * 1e-3) / 1e12,
                                                    "implementation_GBps": p["bytes"] / (p["ms"] * 1e-3) / 1e9}
        families[fam]["layers"] = layers
    if rank == 0 and args.layer_report:
        with open(args.layer_report, "w") as f:
            f.write("# per-layer HIP-event times of the instrumented pass (%d steps, behind the %d un-instrumented headline steps); EXECUTED MFMA FLOP / algorithmic bytes\n" % (prof_steps, args.steps))
            f.write("%-32s %8s %12s %10s %10s\n" % ("name", "launches", "ms/step", "TFLOP/s", "GB/s(alg)"))
            for name in sorted(ctx.profile_names()):
                p = ctx.profile_read(name)
                if p["ms"] <= 0:
                    continue
                f.write("%-32s %8d %12.4f %10.2f %10.1f\n" % (name, p["launches"], p["ms"] / prof_steps,
                                                            p["flops"] / (p["ms"] * 1e-3) / 1e12,
                                                            p["bytes"] / (p["ms"] * 1e-3) / 1e9))
    return {
        "timing": {"ms_per_step_instrumented": 1e3 * elapsed_prof / prof_steps, "instrumented_steps": prof_steps,
                   "note": "kernels / roofline come from the separate instrumented pass (a HIP event pair around each of ~280 launches per step)"},
        "dtype_detail": (("fp32 storage, fp32 accumulation everywhere; the Winograd-form and 1x1 layers' GEMMs form each fp32 product from THREE fp16 MFMA "
                          "partial products (lo*hi + hi*lo + hi*hi) of 2-term split operands: x * 2^s = hi + lo with hi = fp16(x 2^s), lo = fp16(x 2^s - hi), "
                          "|x 2^s - hi - lo| <= 2^-23 |x 2^s| and zero for three elements in four; s per tensor from its MEASURED max |x| (taken by the "
                          "producing kernel's epilogue), per Winograd position for the weights; accumulators scaled back by the exact inverse power of two.  "
                          "Error against float64 at every benched GEMM shape: rms 5.5e-8 / max 1.0e-6 of sum |u||v| -- below the six-product bf16 form "
                          "(6.8e-8 / 1.1e-6) and the fp32 library GEMM (8.7e-8 / 1.6e-6) on the same data, asserted in pytest -m gpu "
                          "(test_split_bf16_gemm_benched_shapes_against_float64; profiles/parity_r06_gemm_split_f64.txt).  extra.track_bf16x3 / "
                          "extra.track_fp32_mfma_only: the same step in the round-5 form and on the fp32 MFMA instruction only") if s3_h2 else
                         ("fp32 storage, fp32 accumulation everywhere; the F(6x6,3x3) layers' GEMMs form each fp32 product from six bf16 MFMA "
                          "partial products of 3-term split operands (x = x1 + x2 + x3, exact to 2^-25 |x|): error against float64 no "
                          "larger than the fp32 MFMA path's (DT_S3=0), which the parity tests assert")) if s3["ms"] > 0 else
                        "fp32 storage, fp32 MFMA arithmetic, fp32 accumulation",
        "roofline": None if dominant is None else {
            "bound": "mfma",
            # the four contract fields describe ONE family -- the one with the most time in the step -- and nothing else;
            # every other figure of a family lives in families[<name>], computed from that family's own launches only
            "kernel": families[dominant]["kernel"] + " -- " + families[dominant]["instruction"],
            "dominant_family": dominant,
            "achieved": families[dominant]["achieved"], "peak": families[dominant]["peak_tflops"], "unit": "TFLOP/s",
            "frac": families[dominant]["frac"],
            "traffic": families[dominant]["traffic_bytes_per_launch"],
            "traffic_unit": "bytes per launch of the dominant family (FETCH_SIZE x in-run calibration + WRITE_SIZE; beyond-L2, incl. Infinity Cache hits)",
            "traffic_source": os.path.relpath(tr[0], ROOT) if tr is not None else None,
            "traffic_per_step": tr[1].get("traffic_bytes_per_step") if tr is not None else None,
            "families": families, "transforms": transforms,
            "frac_whole_conv_path": conv_path_pipe_frac,
            "whole_conv_path": {"executed_fp32_mfma_tflop_per_step": conv_path_flops / steps / 1e12,
                                "executed_bf16_mfma_tflop_per_step": conv_path_bf16 / steps / 1e12,
                                "fp32_equivalent_tflops": ((conv_path_flops + s3["flops"] / s3_products + c3h2["flops"] / 3.0 + (conv1["flops"] / 3.0 if conv1_bf16 else 0.0)) / (conv_path_ms * 1e-3) / 1e12)
                                if conv_path_ms > 0 else None,
                                "ms_per_step": conv_path_ms / steps,
                                "direct_form_tflop_per_step": direct_form_all / steps / 1e12,
                                "direct_form_tflops": (direct_form_all / (conv_path_ms * 1e-3) / 1e12) if conv_path_ms > 0 else None,
                                "direct_form_bytes_per_step": direct_form_bytes_all / steps,
                                "implementation_bytes_per_step": (s3["bytes"] + ig["bytes"] + wino_in["bytes"] + wino_out["bytes"] + fused["bytes"] + c3h2["bytes"] + conv1["bytes"]) / steps},
            "note": "achieved / peak / frac / traffic = the DOMINANT kernel family (most time in the step): MFMA FLOPs its launches execute / "
                    "their HIP-event time, against the dense peak of the instruction it issues (pipe utilisation, <= 1). Per family "
                    "(families.*): executed = FLOPs on the matrix pipe; algorithmic = SURVEY.md 8d direct-form FLOPs (2MKN of the "
                    "reference's layer) of the layers THAT family's launches computed -- the 3x3 layers run in Winograd form "
                    "(F(6x6,3x3): 1.78 multiplies per output instead of 9; fused F(4x4,3x3): 2.25), so achieved_algorithmic exceeds "
                    "achieved; wino_gemm_s3 carries every fp32 operand as two fp16 terms of the scaled operand (three bf16 terms under DT_S3_H2=0) and forms each product from three (six) 16-bit "
                    "MFMA partial products with fp32 accumulation (fp32 accuracy, tests/test_gpu_parity.py::"
                    "test_split_bf16_gemm_benched_shapes_against_float64): fp32_equivalent_tflops = executed / mfma_products_per_multiply. "
                    "implementation_* = bytes the kernels move by their own count (V + U + M' for the GEMMs); traffic_* = PMC "
                    "measurement (profiles/). transforms = the HBM-bound Winograd transform kernels around the GEMMs. "
                    "frac_whole_conv_path = time the matrix pipe needs at its peaks for everything the conv path executes "
                    "(16-bit FLOPs / 2500 + fp32 FLOPs / 157.3) / the conv path's time incl. transforms."},
        "kernels": kern
    }


def main():
    # the classes print a model summary like Keras does; stdout must carry ONLY the JSON line
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):
        out = _run()
    if out is not None:
        print(json.dumps(out), flush=True)


def _run():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--prof-steps", type=int, default=5, help="steps of the separate instrumented pass (per-kernel HIP events) behind the timed steps")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["track", "detect", "tiny"], default="track")
    ap.add_argument("--seqs", type=int, default=32, help="sequences per step (tiny)")
    ap.add_argument("--clips", type=int, default=48, help="clips per GPU per step (track)")
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--graphs", dest="graphs", action="store_true", default=True,
                    help="dt_graph_enable for the timed steps: hipGraph replay of the detector trunk / recurrences (default; the instrumented pass behind them runs plain launches)")
    ap.add_argument("--no-graphs", dest="graphs", action="store_false", help="plain launches in the timed steps too")
    ap.add_argument("--boxes", type=int, default=32, help="boxes/frame the synthetic tracker head is calibrated to (track)")
    ap.add_argument("--batch", type=int, default=8, help="frames per step (detect)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--h2d", action="store_true", help="also copy the frames from pinned host memory every step (PCIe-inclusive rate; never the headline value)")
    ap.add_argument("--cpu-frames", type=int, default=30)
    ap.add_argument("--shard", choices=["clip", "frame"], default="clip",
                    help="N>1 (track): clip = each rank owns --clips whole clips (weak scaling, no data-path collective); "
                         "frame = --clips clips in TOTAL, every rank runs the detector on its time steps of all of them, "
                         "per-frame rows all-gathered, recurrence on each clip's owner (strong scaling; configs[4])")
    ap.add_argument("--no-extra", action="store_true", help="skip the configs[1] extra block")
    ap.add_argument("--layer-report", default=None, help="write a per-layer table (HIP-event times) to this file (needs --full)")
    ap.add_argument("--full", action="store_true",
                    help="behind the headline steps: the instrumented per-kernel pass (kernels, roofline), the extra configurations and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    args = ap.parse_args()
    if args.layer_report and not args.full:
        ap.error("--layer-report comes from the instrumented pass: add --full")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # typed as a plain command: become the launcher -- one rank per GPU of this node under torch.distributed.run
        # (backend nccl = RCCL unless DT_DIST_BACKEND says otherwise); rank 0 of the child job prints the JSON line to
        # the stdout this process inherited
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        rc = subprocess.call(cmd, env=env, stdout=sys.__stdout__, stderr=sys.__stderr__)
        if rc != 0:
            sys.exit(rc)
        return None
    rank, world, local = init_from_env()
    assert world == args.gpus, "--gpus %d but WORLD_SIZE=%d: launch with torchrun --nproc-per-node %d, or run " \
                               "`python bench.py --gpus %d` without a launcher" % (args.gpus, world, args.gpus, args.gpus)
    assert torch.cuda.is_available(), "bench.py needs an MI355X; there is no CPU fallback"
    device = torch.device("cuda", torch.cuda.current_device())
    H = W = args.size

    if args.workload == "track":
        frame_shard = args.shard == "frame" and world > 1
        # frame-shard: ONE set of --clips clips for the whole job; a rank keeps only its own time steps of them resident
        # (sharded ingest: t mod N = rank) once the head is calibrated
        frames = make_frames(args.clips, args.T, H, W, device, seed0=42 + (0 if frame_shard else 100 * rank))
        trk, blob, tw = build_tracker(H, W, args.T, args.boxes, frames)
        if frame_shard:
            from parallel import frame_shard_times
            frames = frames[:, frame_shard_times(args.T, rank, world)].contiguous()
        xstats = {}
        ctx = trk.model.ctx
        frames_per_step = args.clips * args.T / (world if frame_shard else 1)
        gflop_per_frame = GFLOP_TRACK_416 * (H * W) / (416.0 * 416.0)

        host_frames = frames.cpu().pin_memory() if args.h2d else None

        def step():
            src = frames
            if host_frames is not None:
                frames.copy_(host_frames, non_blocking=True)     # same stream: serialised in front of the step
            xstats.clear()
            if frame_shard:
                return track_clips_frame_sharded(trk, src, cap=max(128, 2 * args.boxes), T=args.T, stats=xstats)
            res = trk.track_clips(src, cap=max(128, 2 * args.boxes))
            if world > 1:
                res = gather_detections(res, n_clips_max=args.clips, ctx=ctx, stats=xstats)
            return res
    elif args.workload == "tiny":
        # BASELINE.json configs[3]: TinyTracker (ROLO-style) over 64-frame sequences, FRAME-sharded:
        # every rank runs detector + pooling on its slice of the time axis of all sequences, the
        # small per-frame rows are all-gathered, the LSTM over T runs replicated.  Strong scaling.
        from models_tracking.TinyTracker import TinyTracker
        from parallel import gather_frame_rows
        C, T = 80, 64
        assert T % world == 0
        blob = synth.synth_darknet_blob(C, seed=1234)
        det = KerasYOLO({'LABELS': KerasYOLO.LABELS_COCO, 'BATCH_SIZE': 4, 'IMAGE_H': H, 'IMAGE_W': W,
                         'GRID_H': H // 32, 'GRID_W': W // 32}, weights=blob)
        ctx = det.model.ctx
        cfg = {"model_tracker": {"name": "TinyTracker", "lstm_units": 512, "sequence_length": T},
               "train": {"pool": "Global", "batch_size": 4}}
        tt = TinyTracker(cfg, feature_dims=(H // 16, W // 16, 512), weights=synth.synth_tiny_weights(512), ctx=ctx)
        t_loc = T // world
        frames = make_frames(args.seqs, t_loc, H, W, device, seed0=42 + 100 * rank)
        frames_per_step = args.seqs * t_loc
        gflop_per_frame = GFLOP_DETECT_416_C80 * (H * W) / (416.0 * 416.0)
        tw = None
        xstats = {}

        def step():
            rows, _ = tt.frame_rows(frames.reshape(args.seqs * t_loc, H, W, 3), det)
            rows = gather_frame_rows(rows.reshape(args.seqs, t_loc, -1).contiguous())
            return ctx.tiny_sequence(rows)
    else:
        C = 80
        blob = synth.synth_darknet_blob(C, seed=1234)
        det = KerasYOLO({'LABELS': KerasYOLO.LABELS_COCO, 'BATCH_SIZE': args.batch, 'IMAGE_H': H, 'IMAGE_W': W,
                         'GRID_H': H // 32, 'GRID_W': W // 32}, weights=blob)
        ctx = det.model.ctx
        frames = make_frames(1, args.batch, H, W, device, seed0=42 + 100 * rank)[0].contiguous()
        frames_per_step = args.batch
        gflop_per_frame = GFLOP_DETECT_416_C80 * (H * W) / (416.0 * 416.0)
        tw = None
        xstats = {}

        def step():
            return det.detect(frames)

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if args.graphs:
        ctx.graph_enable(True)        # captured during the warm-up steps (second call per shape), replayed afterwards
    res = None
    for _ in range(max(args.warmup, 3) if args.graphs else args.warmup):
        res = step()
    sync_all()
    # ---- the contract number: K steps with NO per-launch instrumentation (HIP events around every launch cost ~1 %) ----
    ctx.profile_reset()
    ctx.profile_enable(False)
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    sync_all()
    elapsed = time.perf_counter() - t0
    per_rank_ms = None
    if world > 1:
        rec = [None] * world
        dist.all_gather_object(rec, {"rank": rank, "ms_per_step": 1e3 * elapsed / args.steps})      # every rank's own clock, both shard modes
        per_rank_ms = rec
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, res)
    full = instrumented_report(args, ctx, step, sync_all, rank) if args.full else None

    # frame-shard: where each rank spent the last step (with --full: the last instrumented one) -- the part spread over all ranks (detector + input projection) vs the
    # owner stage (row wait + recurrence + decode on the clips it owns; a rank that owns none idles there)
    stage_ms = None
    if args.workload == "track" and args.shard == "frame" and world > 1:
        mine = frame_shard_stage_ms(xstats)
        rec = [None] * world
        dist.all_gather_object(rec, {"rank": rank, "clips_owned": xstats.get("clips_owned"),
                                     "sharded_stage_ms": mine[0] if mine else None, "owner_stage_ms": mine[1] if mine else None})
        stage_ms = rec

    boxes_per_frame = None
    if args.workload == "track" and res is not None and isinstance(res, dict):
        boxes_per_frame = float(res["counts"].float().mean().item())

    if rank == 0:
        total_frames = frames_per_step * world * args.steps
        fps = total_frames / elapsed
        out = {
            "metric": {"track": "frames/sec detect+track @416x416", "detect": "frames/sec detect @416x416",
                       "tiny": "frames/sec detect + single-object LSTM track @416x416"}[args.workload],
            "value": fps, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "timing": {"headline": "%d steps without per-launch events (profile off)%s" % (args.steps, ", detector trunk and recurrences replayed as hipGraphs (dt_graph_enable)" if args.graphs else ", plain launches"),
                       "hipgraph": bool(args.graphs)},
            "scaling": "strong" if (args.workload == "tiny" or (args.workload == "track" and args.shard == "frame" and world > 1)) else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": ("BASELINE.json configs[2]: MultiObjDetTracker (YOLOv2 C=12 + ConvLSTM2D(512) + 1x1 "
                                    "+ decode/NMS + track ids), %d clips x %d frames per GPU per step, %dx%d uint8; the synthetic head is calibrated "
                                    "to %d CANDIDATE boxes per frame, of which about 20 survive NMS (config.boxes_per_frame: measured).  The step computes the model's "
                                    "TRACKING output, the one MultiObjDetTracker.predict reads (MultiObjDetTracker.py:307: output[0]); conv_23 is folded into the "
                                    "ConvLSTM input projection's weights and the detection grid (output[1]) is not materialised -- "
                                    "extra.track_with_detection_output times the step that writes both"
                                    % (args.clips, args.T, H, W, args.boxes)) if args.workload == "track" else
                       ("BASELINE.json configs[1]: YOLOv2 C=80 forward + decode/NMS, batch %d, %dx%d uint8"
                        % (args.batch, H, W)) if args.workload == "detect" else
                       ("BASELINE.json configs[3]: TinyTracker, %d sequences x 64 frames, frame-sharded x%d: YOLOv2 C=80 "
                        "+ act_13 global max-pool + decode/top box per frame, LSTM(512)+Dense(4) over T" % (args.seqs, world)),
                       "frames_per_step_per_gpu": frames_per_step,
                       "parallelism": ("frame-shard x%d (detector on t mod N, rows all-gathered, recurrence on the clip owner)" % world)
                       if (args.workload == "track" and args.shard == "frame" and world > 1) else "clip-shard x%d" % world,
                       "gflop_per_frame": gflop_per_frame, "boxes_per_frame": boxes_per_frame},
            "whole_path_tflops": fps * gflop_per_frame / 1e3, "h2d_included": bool(args.h2d),
            "ranks_seen": dist.get_world_size() if (world > 1 and dist.is_initialized()) else 1,
            "exchange_bytes_received_per_step_rank0": int(xstats.get("bytes_received", 0)),
            "frame_shard_stage_ms_per_rank": stage_ms, "ms_per_step_per_rank": per_rank_ms,
        }
        if full is not None:
            out["timing"].update(full.pop("timing"))
            out.update(full)
        if args.full and world == 1 and not args.no_extra and args.workload == "track":
            import gc
            out["extra"] = {}
            for key, fn in (("detect_batch8", lambda: detect_batch8_extra(device, H, W, seed0=4242)),
                            ("track_608_128boxes", lambda: track_extra(device, 608, 24, args.T, 128)),
                            ("tiny_T64", lambda: tiny_extra(device, H, W, 32)),
                            # ONE clip per call (the live-camera shape of configs[2]): the latency of a 30-frame clip through detector + ConvLSTM + decode +
                            # association under the library's default policy for that size (fp16 form from 20 frames per forward, recurrent step in
                            # Winograd form on the split kernel from one clip: profiles/r06_experiments.txt section 10)
                            ("track_1_clip", lambda: track_extra(device, args.size, 1, args.T, args.boxes, steps=20,
                                                                 what="BASELINE.json configs[2] with ONE clip per call: 1 x %d frames %dx%d (latency of a clip)" % (args.T, args.size, args.size))),
                            ("track_8_clips", lambda: track_extra(device, args.size, 8, args.T, args.boxes, steps=10,
                                                                  what="BASELINE.json configs[2] with 8 clips per call: 8 x %d frames %dx%d" % (args.T, args.size, args.size))),
                            # the headline workload with hipGraph replay of the detector trunk and the recurrence (dt_graph_enable): no
                            # per-launch events are possible inside a replayed graph, so the headline number (which carries them) runs without
                            ("track_plain_launches" if args.graphs else "track_hipgraph",
                             lambda: track_extra(device, H, args.clips, args.T, args.boxes, steps=args.steps, graphs=not args.graphs,
                                                 what="the headline workload (BASELINE.json configs[2], %d clips x %d frames) %s" % (
                                                     args.clips, args.T, "with plain launches instead of hipGraph replay" if args.graphs else
                                                     "with dt_graph_enable: the detector trunk and the ConvLSTM recurrence replayed as hipGraphs"))),
                            # the headline workload with the split-bf16 GEMMs switched off (DT_S3=0: v_mfma_f32_32x32x2_f32
                            # everywhere), same run, same clock: what the bf16-pipe arithmetic buys
                            ("track_fp32_mfma_only", lambda: track_extra(
                                device, args.size, args.clips, args.T, args.boxes, env={"DT_S3": "0"},
                                what="the headline workload (BASELINE.json configs[2], %d clips x %d frames) with DT_S3=0: every GEMM on "
                                     "the fp32 MFMA instruction" % (args.clips, args.T))),
                            # ... in round 5's operand form: three bf16 terms, six MFMA products per multiply
                            ("track_bf16x3", lambda: track_extra(
                                device, args.size, args.clips, args.T, args.boxes, env={"DT_S3_H2": "0"}, steps=args.steps, graphs=args.graphs,
                                what="the headline workload (BASELINE.json configs[2], %d clips x %d frames) with DT_S3_H2=0: the split GEMMs in the "
                                     "three-term bf16 form (six products per multiply), same run" % (args.clips, args.T))),
                            # ... writing BOTH outputs of the reference's model (tracking and detection grids: conv_23 launched, two-output forward)
                            ("track_with_detection_output", lambda: track_extra(
                                device, args.size, args.clips, args.T, args.boxes, steps=args.steps, graphs=args.graphs, want_det=True,
                                what="the headline workload (BASELINE.json configs[2], %d clips x %d frames) computing the model's detection output "
                                     "too (model.forward(want_det=True): conv_23 is launched and its grid written next to the tracking grid)" % (args.clips, args.T)))):
                out["extra"][key] = fn()
                gc.collect()                      # each extra owns a context with its own workspaces: release them
                torch.cuda.empty_cache()
        if args.full and world == 1 and not args.no_cpu_baseline and args.workload == "track":
            from oracle import oracle as orc
            orc.lib()
            variants = cpu_baseline_track(blob, tw, H, W, args.cpu_frames)
            host = variants.pop("_host")
            best = max(variants, key=lambda k: variants[k][0])
            out["cpu_baseline"] = {"value": variants[best][0], "unit": "frames/s", "cores": variants[best][2], "kind": "port",
                                   "gflops": variants[best][0] * gflop_per_frame, "gflops_per_thread": variants[best][0] * gflop_per_frame / max(1, variants[best][2]),
                                   "numa_node_cores_bound": host["numa_node_cores_bound"], "physical_cores_in_binding": host["physical_cores_in_binding"],
                                   "limit": ("threads: the sweep's fastest count is the largest tried" if variants[best][2] >= max(host["detector_frames_per_s_by_threads"][best])
                                             else "not threads: %d threads beat every larger count of the sweep -- memory / synchronisation of the frame-sized "
                                                  "convolutions (the 13x13 layers have 169 pixels per frame to share)" % variants[best][2]),
                                   "variant": best, "host_logical_cores": host["host_logical_cores"], "affinity_cores": host["affinity_cores"],
                                   "thread_sweep_detector_frames_per_s": host["detector_frames_per_s_by_threads"],
                                   "variants": {k: {"frames_per_s": v[0], "seconds": v[1], "threads": v[2]} for k, v in variants.items()},
                                   "sample": "CPU restatement of the graph (NOT Keras/TF, which cannot run here), the fastest of "
                                             "oracle/oracle.c (C + OpenMP) and oracle/torch_cpu.py (ATen/oneDNN, NHWC and NCHW tensors; the clip's "
                                             "frames go through every layer as ONE batch): 1 clip x %d "
                                             "frames %dx%d through detector+ConvLSTM+1x1+decode+association after a warm-up and "
                                             "a thread-count sweep without early exit, every thread bound to the cores of one NUMA node "
                                             "(cores = threads of the reported variant), %.1f s"
                                             % (args.cpu_frames, H, W, variants[best][1])}
    else:
        out = None
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
