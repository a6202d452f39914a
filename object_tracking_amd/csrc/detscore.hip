// detscore.hip -- detection scoring (BUILD-DEFINED, DESIGN.md "Detection scoring"): per-class average precision of a detector's boxes
// against ground truth, by the VOC devkit's match.  Integers out (and the IoU of each match); the ratios are taken on the host.
//
// detect_match_kernel: one 64-lane workgroup per frame, lanes over rows in passes of 64.
//   1. the ground-truth rows are staged in LDS; lane = detection walks them and keeps, among the rows of its label, the one of the
//      largest IoU (a strict comparison keeps the lowest g).  The argmax ignores claims, so nothing needs a serial walk:
//   2. detection i is a duplicate at threshold k exactly when a detection that stands before it in the frame's score order (higher
//      score, or equal score and lower row) has the same best row and an IoU >= thr[k] -- the first such detection claimed the row.
//      So each lane takes the largest IoU over the detections before it that share its best row, once, and compares it per threshold.
//      (The rule's test is "iou < thr": a NaN IoU, 0 / 0 of two boxes without area, passes it and claims; it counts as +inf here.)
//   LDS, in words: 6 * gcap (x, y, w, h, label, ignore) + 3 * cap (score, best row, IoU).
// detect_rank: detect_prefix_kernel (rows in use before each frame; zeroes the totals), detect_compact_kernel (the rows in use, in
//   flat-index order: score, label, the states of all thresholds two bits each; -1 into rank / ctp of every other row; ngt),
//   detect_rank_kernel (one thread per row in use; the other rows stream through LDS in tiles; per threshold it counts the ranked
//   rows and the TPs of its label that stand before it).  Integer atomics only, for the per-class totals.
//
// Out of scope, on purpose: COCO's match (best UNCLAIMED row, crowd regions), area ranges and max-detections cuts, per-class score
// thresholds, label-free AP.
//
// This translation unit is compiled with -ffp-contract=off: the IoU is bbox_iou_ref's float32 bits (dt_internal.h).
#include "dt_internal.h"

#define DETSCORE_LDS_LIMIT (160 * 1024)
#define RANK_THREADS 256
#define RANK_CHUNK 15            // entries added into 4-bit fields before they are flushed into the counters

// a label that takes part is an integer value in 0..NC-1
__device__ __forceinline__ bool label_ok(float l, int NC) { return l >= 0.0f && l < (float)NC && l == floorf(l); }

__global__ __launch_bounds__(64) void detect_match_kernel(DetMatchArgs p)
{
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int cap = p.cap, gcap = p.gcap, n_thr = p.n_thr;
    float *gx = smem_f, *gy = gx + gcap, *gw = gy + gcap, *gh = gw + gcap, *gl = gh + gcap;
    int *gf = reinterpret_cast<int *>(gl + gcap);
    float *ds = reinterpret_cast<float *>(gf + gcap);
    int *db = reinterpret_cast<int *>(ds + cap);
    float *di = reinterpret_cast<float *>(db + cap);

    const int nd = min(max(p.det_counts[b], 0), cap), ng = min(max(p.gt_counts[b], 0), gcap);
    const float *gtb = p.gt_boxes + (long long)b * gcap * DT_BOX_FLOATS;
    const float *dtb = p.det_boxes + (long long)b * cap * DT_BOX_FLOATS;
    const long long row0 = (long long)b * cap, plane = (long long)p.B * cap;

    for (int g = lane; g < ng; g += 64) {
        const float *q = gtb + (long long)g * DT_BOX_FLOATS;
        const float4 v = *reinterpret_cast<const float4 *>(q);
        gx[g] = v.x; gy[g] = v.y; gw[g] = v.z; gh[g] = v.w; gl[g] = q[5];
        gf[g] = p.gt_flags ? (p.gt_flags[(long long)b * gcap + g] & 1) : 0;
    }
    __syncthreads();
    // ---- 1. the best candidate of every detection (db: -1 none, -2 the row takes no part) ----
    for (int i = lane; i < cap; i += 64) {
        int bj = -1;
        float bi = 0.0f;
        if (i < nd) {
            const float *q = dtb + (long long)i * DT_BOX_FLOATS;
            const float4 v = *reinterpret_cast<const float4 *>(q);
            const float l = q[5];
            if (label_ok(l, p.NC)) {
                for (int g = 0; g < ng; ++g) {
                    if (gl[g] != l) continue;
                    const float iou = bbox_iou_ref(gx[g], gy[g], gw[g], gh[g], v.x, v.y, v.z, v.w);
                    if (bj < 0 || iou > bi) { bj = g; bi = iou; }
                }
                db[i] = bj;
            } else {
                db[i] = -2;
            }
            ds[i] = q[p.score_at];
            di[i] = bi;
        }
        p.best[row0 + i] = bj;
        p.iou[row0 + i] = bi;
    }
    __syncthreads();
    // ---- 2. the states: the largest IoU among the detections before this one that share its best row decides "claimed" ----
    for (int i = lane; i < cap; i += 64) {
        int mb = -2;
        float mi = 0.0f, prior = -1.0f;
        bool ign = false;
        if (i < nd) {
            mb = db[i];
            mi = di[i];
            if (mb >= 0) {
                const float s = ds[i];
                ign = gf[mb] != 0;
                for (int j = 0; j < nd; ++j) {
                    const float sj = ds[j];
                    const float ij = di[j];
                    if (db[j] == mb && (sj > s || (sj == s && j < i))) prior = fmaxf(prior, ij != ij ? INFINITY : ij);
                }
            }
        }
        for (int k = 0; k < n_thr; ++k) {
            const float t = p.thr[k];
            int st;
            if (mb == -2) st = -1;
            else if (mb < 0 || mi < t) st = 0;                 // (a NaN IoU -- two boxes without area -- is below no threshold)
            else if (ign) st = 2;
            else st = prior >= t ? 0 : 1;
            p.state[(long long)k * plane + row0 + i] = st;
        }
    }
}

size_t detect_match_lds_bytes(int cap, int gcap) { return ((size_t)3 * (size_t)cap + (size_t)6 * (size_t)gcap) * sizeof(int); }

int launch_detect_match(hipStream_t st, const DetMatchArgs &a)
{
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(detect_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       DETSCORE_LDS_LIMIT) != hipSuccess;
        }))
        return 1;
    hipLaunchKernelGGL(detect_match_kernel, dim3((unsigned)a.B), dim3(64), detect_match_lds_bytes(a.cap, a.gcap), st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rank
// ---------------------------------------------------------------------------------------------------------------------------------
// hist[c] += the number of lanes with `on` and label c, one atomic per distinct label of the wavefront.  Every lane of the wavefront
// must call it (on = false where it has nothing to add).
__device__ __forceinline__ void wave_hist_add(int *hist, int c, bool on)
{
    unsigned long long todo = __ballot(on);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int c0 = __shfl(c, lead);
        const unsigned long long same = __ballot(on && c == c0);
        if (lane == lead) atomicAdd(hist + c0, __popcll(same));
        todo &= ~same;
    }
}

// one workgroup: offsets[b] = sum of min(count, cap) over the frames before b, offsets[B] = the rows in use; the totals are zeroed
__global__ __launch_bounds__(RANK_THREADS) void detect_prefix_kernel(DetRankArgs p)
{
    __shared__ int part[RANK_THREADS];
    const int tid = threadIdx.x;
    for (int i = tid; i < p.NC; i += RANK_THREADS) p.ngt[i] = 0;
    for (long long i = tid; i < (long long)p.n_thr * p.NC; i += RANK_THREADS) { p.ndet[i] = 0; p.ntp[i] = 0; }
    int running = 0;
    for (int base = 0; base < p.B; base += RANK_THREADS) {
        const int b = base + tid;
        const int v = b < p.B ? min(max(p.det_counts[b], 0), p.cap) : 0;
        part[tid] = v;
        __syncthreads();
        for (int d = 1; d < RANK_THREADS; d <<= 1) {
            const int add = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        if (b < p.B) p.offsets[b] = running + part[tid] - v;
        running += part[RANK_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) p.offsets[p.B] = running;
}

// thread = flat row of [B][cap] and of [B][gcap]
__global__ __launch_bounds__(RANK_THREADS) void detect_compact_kernel(DetRankArgs p)
{
    const long long f = (long long)blockIdx.x * RANK_THREADS + threadIdx.x;
    const long long plane = (long long)p.B * p.cap;
    if (f < plane) {
        const int b = (int)(f / p.cap), i = (int)(f - (long long)b * p.cap);
        if (i < min(max(p.det_counts[b], 0), p.cap)) {
            const float *q = p.det_boxes + f * DT_BOX_FLOATS;
            const float l = q[5];
            const bool ok = label_ok(l, p.NC);
            unsigned w = 0xffffffffu;                        // state -1 reads as 3 in every field
            if (ok) {
                w = 0u;
                for (int k = 0; k < DT_DETSCORE_MAX_THR; ++k) {
                    const unsigned s = k < p.n_thr ? ((unsigned)p.state[(long long)k * plane + f] & 3u) : 3u;
                    w |= s << (2 * k);
                }
            }
            const int r = p.offsets[b] + i;
            p.c_score[r] = q[p.score_at];
            p.c_label[r] = ok ? (int)l : -1;
            p.c_state[r] = w;
            p.c_flat[r] = (int)f;
        } else {
            for (int k = 0; k < p.n_thr; ++k) {
                p.rank[(long long)k * plane + f] = -1;
                p.ctp[(long long)k * plane + f] = -1;
            }
        }
    }
    // ground-truth rows per label, the ignored ones left out
    int c = 0;
    bool on = false;
    if (f < (long long)p.B * p.gcap) {
        const int b = (int)(f / p.gcap), g = (int)(f - (long long)b * p.gcap);
        if (g < min(max(p.gt_counts[b], 0), p.gcap)) {
            const float l = p.gt_boxes[f * DT_BOX_FLOATS + 5];
            if (label_ok(l, p.NC) && !(p.gt_flags && (p.gt_flags[f] & 1))) {
                on = true;
                c = (int)l;
            }
        }
    }
    wave_hist_add(p.ngt, c, on);
}

// thread = row in use r.  For every other row j of its label that stands before it (higher score, or equal score and j < r: the rows
// are in flat-index order) and every threshold: is j ranked (state 0 or 1), is it a TP.  The two bits per threshold of j's state word
// turn into one "ranked" and one "TP" bit each; those are added up in 4-bit fields, eight thresholds to a word, and flushed into the
// 2 x 16 counters every RANK_CHUNK rows.
__global__ __launch_bounds__(RANK_THREADS) void detect_rank_kernel(DetRankArgs p)
{
    __shared__ float t_score[RANK_THREADS];
    __shared__ int t_label[RANK_THREADS];
    __shared__ unsigned t_state[RANK_THREADS];
    const int N = p.offsets[p.B];
    if ((long long)blockIdx.x * RANK_THREADS >= N) return;            // the whole workgroup leaves
    const int tid = threadIdx.x;
    const int r = blockIdx.x * RANK_THREADS + tid;
    const bool live = r < N;
    const float s = live ? p.c_score[r] : 0.0f;
    const int c = live ? p.c_label[r] : -1;
    const unsigned w = live ? p.c_state[r] : 0xffffffffu;
    const int cm = c >= 0 ? c : -3;                                   // matches no tile entry
    int cr[DT_DETSCORE_MAX_THR], ct[DT_DETSCORE_MAX_THR];
#pragma unroll
    for (int k = 0; k < DT_DETSCORE_MAX_THR; ++k) { cr[k] = 0; ct[k] = 0; }

    for (int base = 0; base < N; base += RANK_THREADS) {
        const int j = base + tid;
        t_score[tid] = j < N ? p.c_score[j] : 0.0f;
        t_label[tid] = j < N ? p.c_label[j] : -2;
        t_state[tid] = j < N ? p.c_state[j] : 0xffffffffu;
        __syncthreads();
        for (int e0 = 0; e0 < RANK_THREADS; e0 += RANK_CHUNK) {
            const int e1 = min(e0 + RANK_CHUNK, RANK_THREADS);
            unsigned ra = 0u, rb = 0u, ta = 0u, tb = 0u;
            for (int e = e0; e < e1; ++e) {
                const float sj = t_score[e];
                const bool before = t_label[e] == cm && (sj > s || (sj == s && base + e < r));
                const unsigned wj = before ? t_state[e] : 0xffffffffu;
                const unsigned rk = ~(wj >> 1) & 0x55555555u;         // bit 2k: state 0 or 1 at threshold k
                const unsigned tp = wj & rk;                          // ... state 1
                ra += rk & 0x11111111u;                               // thresholds 0, 2, 4, ...: field k / 2
                rb += (rk >> 2) & 0x11111111u;                        // thresholds 1, 3, 5, ...
                ta += tp & 0x11111111u;
                tb += (tp >> 2) & 0x11111111u;
            }
#pragma unroll
            for (int k = 0; k < DT_DETSCORE_MAX_THR; ++k) {
                cr[k] += (int)((((k & 1) ? rb : ra) >> (4 * (k >> 1))) & 15u);
                ct[k] += (int)((((k & 1) ? tb : ta) >> (4 * (k >> 1))) & 15u);
            }
        }
        __syncthreads();
    }
    const long long plane = (long long)p.B * p.cap;
    const int f = live ? p.c_flat[r] : 0;
#pragma unroll
    for (int k = 0; k < DT_DETSCORE_MAX_THR; ++k) {
        if (k < p.n_thr) {                                            // uniform
            const unsigned st = (w >> (2 * k)) & 3u;
            const bool ranked = live && st < 2u, tp = live && st == 1u;
            if (live) {
                p.rank[(long long)k * plane + f] = ranked ? cr[k] : -1;
                p.ctp[(long long)k * plane + f] = ranked ? ct[k] + (tp ? 1 : 0) : -1;
            }
            wave_hist_add(p.ndet + (long long)k * p.NC, c, ranked);
            wave_hist_add(p.ntp + (long long)k * p.NC, c, tp);
        }
    }
}

size_t detect_rank_ws_bytes(int B, int cap)
{
    const size_t rows = (size_t)B * (size_t)cap;
    return (((size_t)B + 1 + 3) / 4 * 4 + 4 * rows) * sizeof(int);
}

void detect_rank_ws_carve(DetRankArgs &a, void *ws)
{
    const size_t rows = (size_t)a.B * (size_t)a.cap;
    a.offsets = static_cast<int *>(ws);
    a.c_score = reinterpret_cast<float *>(a.offsets + ((size_t)a.B + 1 + 3) / 4 * 4);
    a.c_label = reinterpret_cast<int *>(a.c_score + rows);
    a.c_state = reinterpret_cast<unsigned *>(a.c_label + rows);
    a.c_flat = reinterpret_cast<int *>(a.c_state + rows);
}

int launch_detect_rank(hipStream_t st, const DetRankArgs &a)
{
    hipLaunchKernelGGL(detect_prefix_kernel, dim3(1), dim3(RANK_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return 1;
    if (a.B == 0) return 0;
    const long long rows = (long long)a.B * a.cap, grows = (long long)a.B * a.gcap;
    const long long most = rows > grows ? rows : grows;
    hipLaunchKernelGGL(detect_compact_kernel, dim3((unsigned)((most + RANK_THREADS - 1) / RANK_THREADS)), dim3(RANK_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return 1;
    hipLaunchKernelGGL(detect_rank_kernel, dim3((unsigned)((rows + RANK_THREADS - 1) / RANK_THREADS)), dim3(RANK_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
