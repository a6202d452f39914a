// hota.hip -- HOTA scoring (BUILD-DEFINED, DESIGN.md "HOTA scoring"): Luiten et al.'s measure restated on the quantised similarity
// q = (int)(IoU * 2^20), so that every device output is an integer that does not depend on the order of any sum.  Three kernels, 64-lane
// workgroups; the frame's match between the second and the third is dt_assign_max (identity.hip), called by the caller.
//
// hota_align_kernel, one wavefront per clip, frames in sequence.  Per frame:
//   1. the trajectory of every row (open_trajectories, identity scoring's tables and overflow counts);
//   2. lanes cover the hypotheses of ground-truth row g: R[g] = sum_i q[g][i] by a wave reduction, C[i] = sum_g q[g][i] in the word the
//      lane owns (i = lane mod 64), both int64 in LDS;
//   3. the same walk again: a pair with q > 0 adds c = (q << 20) / (R[g] + C[i] - q) to align[a][b] in global memory (an int64 atomic:
//      repeated ids can make two pairs of a frame hit one word).  q is computed twice, not stored: a [gcap][hcap] tile would not fit.
// LDS, in words: 2 * acap + 2 * bcap (id and boxes of every trajectory) + 9 * gcap + 9 * hcap (x, y, w, h, label, id, trajectory, and
// the int64 R or C).
//
// hota_weights_kernel, one wavefront per (clip, frame): both finished tables are read into LDS, every row looks its id up (an id is in
// the finished table exactly when the alignment gave its boxes a trajectory: tables only grow), and lanes cover the hypotheses of row g:
// W = 1 + (P[a][b] * q) / (2^20 * (n_a + n_b) - P[a][b]) where q > 0, else 0; every word of the [gcap][hcap] tile is stored.
// LDS, in words: 2 * acap + 2 * bcap + 7 * gcap + 7 * hcap.
//
// hota_count_kernel, one wavefront per (clip, frame), lane = ground-truth row: the matched pair's IoU again (the call whose product
// gave q), its level L = the thresholds it reaches, and for L >= 1 the bucket L - 1 gets 1 in tp, q in loc (both through an LDS
// histogram: one global atomic per bucket and frame) and 1 in pairs[a][b].  No dynamic LDS.
// This translation unit is compiled with -ffp-contract=off: the IoU is bbox_iou_ref's float32 bits (dt_internal.h).
#include "dt_internal.h"

#define HOTA_LDS_LIMIT (160 * 1024)

// the quantised similarity: the product is exact (a power of two), the conversion truncates; a NaN IoU is not > 0
__device__ __forceinline__ int hota_q(float iou) { return iou > 0.0f ? __float2int_rz(iou * (float)DT_ASSIGN_IOU_SCALE) : 0; }

// the frame's rows of one side into LDS, lanes over the rows: x, y, w, h, label and id
__device__ __forceinline__ void hota_load_rows(const float *boxes, const int *ids, int n, int id_stride, int label_at, volatile float *x,
                                               volatile float *y, volatile float *w, volatile float *h, volatile float *l, volatile int *id,
                                               int lane)
{
    for (int r = lane; r < n; r += 64) {
        const float *q = boxes + (long long)r * 8;
        const float4 b = *reinterpret_cast<const float4 *>(q);
        x[r] = b.x; y[r] = b.y; w[r] = b.z; h[r] = b.w; l[r] = q[label_at];
        id[r] = ids[(long long)r * id_stride];
    }
}

template <bool ANY>
__global__ __launch_bounds__(64) void hota_align_kernel(HotaArgs p, int resume)
{
    extern __shared__ __attribute__((aligned(16))) int smem_i[];
    const int clip = blockIdx.x, lane = threadIdx.x;
    const int T = p.T, gcap = p.gcap, hcap = p.hcap, acap = p.acap, bcap = p.bcap;
    // the int64 sums first (8-byte aligned), then identity_overlap_kernel's layout: the two tables, the ground truth, the hypotheses
    volatile long long *rsum = reinterpret_cast<volatile long long *>(smem_i), *csum = rsum + gcap;
    volatile int *a_id = reinterpret_cast<volatile int *>(csum + hcap), *a_n = a_id + acap, *b_id = a_n + acap, *b_n = b_id + bcap;
    volatile float *gx = reinterpret_cast<volatile float *>(b_n + bcap), *gy = gx + gcap, *gw = gy + gcap, *gh = gw + gcap, *gl = gh + gcap;
    volatile int *g_id = reinterpret_cast<volatile int *>(gl + gcap), *g_ent = g_id + gcap;
    volatile float *hx = reinterpret_cast<volatile float *>(g_ent + gcap), *hy = hx + hcap, *hw = hy + hcap, *hh = hw + hcap, *hl = hh + hcap;
    volatile int *h_id = reinterpret_cast<volatile int *>(hl + hcap), *h_ent = h_id + hcap;

    const float *gtb = p.gt_boxes + (long long)clip * T * gcap * DT_BOX_FLOATS;
    const int *gtc = p.gt_counts + (long long)clip * T;
    const int *gti = p.gt_ids + (long long)clip * T * gcap;
    const float *hpb = p.hyp_boxes + (long long)clip * T * hcap * 8;
    const int *hpc = p.hyp_counts + (long long)clip * T;
    const int *hpi = p.hyp_ids + (long long)clip * T * hcap * p.id_stride;
    int *sz = p.sizes + (long long)clip * DT_IDENT_INTS;
    int *ta = p.gt_tab + (long long)clip * acap * 2;
    int *tb = p.hyp_tab + (long long)clip * bcap * 2;
    long long *al = p.align + (long long)clip * acap * bcap;   // zero (the launcher's memset), or as the previous chunk left it

    int na = 0, nb = 0;
    int s_frames = 0, s_gt = 0, s_hyp = 0, s_over_a = 0, s_over_b = 0, s_pairs = 0;
    if (resume) {
        s_frames = sz[0]; s_gt = sz[1]; s_hyp = sz[2]; s_over_a = sz[5]; s_over_b = sz[6]; s_pairs = sz[7];
        na = min(max(sz[3], 0), acap);
        nb = min(max(sz[4], 0), bcap);
        for (int e = lane; e < na; e += 64) {
            const int2 r = *reinterpret_cast<const int2 *>(ta + (long long)e * 2);
            a_id[e] = r.x; a_n[e] = r.y;
        }
        for (int e = lane; e < nb; e += 64) {
            const int2 r = *reinterpret_cast<const int2 *>(tb + (long long)e * 2);
            b_id[e] = r.x; b_n[e] = r.y;
        }
    }
    for (int t = 0; t < T; ++t) {
        const int ng = min(max(gtc[t], 0), gcap), nh = min(max(hpc[t], 0), hcap);
        hota_load_rows(gtb + (long long)t * gcap * DT_BOX_FLOATS, gti + (long long)t * gcap, ng, 1, 5, gx, gy, gw, gh, gl, g_id, lane);
        hota_load_rows(hpb + (long long)t * hcap * 8, hpi + (long long)t * hcap * p.id_stride, nh, p.id_stride, p.label_at, hx, hy, hw, hh, hl,
                       h_id, lane);
        for (int i = lane; i < nh; i += 64) csum[i] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // ---- 1. the trajectory of every row ----
        s_over_a += open_trajectories(g_id, g_ent, ng, a_id, a_n, na, acap, lane);
        s_over_b += open_trajectories(h_id, h_ent, nh, b_id, b_n, nb, bcap, lane);
        // q of row g (its box in ax .. al_) against hypothesis i: 0 without a trajectory on the hypothesis' side or with another label
        auto pair_q = [&](float ax, float ay, float aw, float ah, float al_, int i) {
            if (i >= nh || h_ent[i] < 0 || !(ANY || hl[i] == al_)) return 0;
            return hota_q(bbox_iou_ref(ax, ay, aw, ah, hx[i], hy[i], hw[i], hh[i]));
        };
        // ---- 2. the row and column sums of q, lanes over the hypotheses of row g ----
        for (int g = 0; g < ng; ++g) {
            long long r = 0;
            if (g_ent[g] >= 0) {
                const float ax = gx[g], ay = gy[g], aw = gw[g], ah = gh[g], al_ = gl[g];
                for (int i0 = 0; i0 < nh; i0 += 64) {
                    const int i = i0 + lane;
                    const int q = pair_q(ax, ay, aw, ah, al_, i);
                    if (q > 0) { csum[i] = csum[i] + q; r += q; }         // word i belongs to this lane in every pass
                }
                for (int s = 32; s > 0; s >>= 1) r += __shfl_xor(r, s);
            }
            if (lane == 0) rsum[g] = r;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // ---- 3. every pair's share of its row and column, added to its trajectories' alignment ----
        for (int g = 0; g < ng; ++g) {
            const int a = g_ent[g];
            if (a < 0) continue;
            const float ax = gx[g], ay = gy[g], aw = gw[g], ah = gh[g], al_ = gl[g];
            const long long rg = rsum[g];
            long long *row = al + (long long)a * bcap;
            for (int i0 = 0; i0 < nh; i0 += 64) {
                const int i = i0 + lane;
                const int q = pair_q(ax, ay, aw, ah, al_, i);
                if (q > 0) {
                    const long long c = ((long long)q << 20) / (rg + csum[i] - q);       // the divisor is >= q > 0
                    atomicAdd(reinterpret_cast<unsigned long long *>(row + h_ent[i]), (unsigned long long)c);
                }
                s_pairs += __popcll(__ballot(q > 0));
            }
        }
        s_frames += 1; s_gt += ng; s_hyp += nh;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) {
        *reinterpret_cast<int4 *>(sz) = make_int4(s_frames, s_gt, s_hyp, na);
        *reinterpret_cast<int4 *>(sz + 4) = make_int4(nb, s_over_a, s_over_b, s_pairs);
    }
    for (int e = lane; e < acap; e += 64)
        *reinterpret_cast<int2 *>(ta + (long long)e * 2) = e < na ? make_int2(a_id[e], a_n[e]) : make_int2(-1, 0);
    for (int e = lane; e < bcap; e += 64)
        *reinterpret_cast<int2 *>(tb + (long long)e * 2) = e < nb ? make_int2(b_id[e], b_n[e]) : make_int2(-1, 0);
}

// Rows [0, nr) of a frame, ids r_id, against a finished table of nt distinct ids: r_ent[r] becomes the id's row, or -1
__device__ __forceinline__ void find_trajectories(volatile int *r_id, volatile int *r_ent, int nr, volatile int *t_id, int nt, int lane)
{
    for (int r = lane; r < nr; r += 64) {
        const int id = r_id[r];
        int e = -1;
        if (id >= 0)
            for (int k = 0; k < nt; ++k) e = t_id[k] == id ? k : e;
        r_ent[r] = e;
    }
}

template <bool ANY>
__global__ __launch_bounds__(64) void hota_weights_kernel(HotaArgs p)
{
    extern __shared__ __attribute__((aligned(16))) int smem_i[];
    const int clip = blockIdx.x / p.T, t = blockIdx.x % p.T, lane = threadIdx.x;
    const int T = p.T, gcap = p.gcap, hcap = p.hcap, acap = p.acap, bcap = p.bcap;
    volatile int *a_id = smem_i, *a_n = a_id + acap, *b_id = a_n + acap, *b_n = b_id + bcap;
    volatile float *gx = reinterpret_cast<volatile float *>(b_n + bcap), *gy = gx + gcap, *gw = gy + gcap, *gh = gw + gcap, *gl = gh + gcap;
    volatile int *g_id = reinterpret_cast<volatile int *>(gl + gcap), *g_ent = g_id + gcap;
    volatile float *hx = reinterpret_cast<volatile float *>(g_ent + gcap), *hy = hx + hcap, *hw = hy + hcap, *hh = hw + hcap, *hl = hh + hcap;
    volatile int *h_id = reinterpret_cast<volatile int *>(hl + hcap), *h_ent = h_id + hcap;

    const long long frame = (long long)clip * T + t;
    const int *sz = p.sizes + (long long)clip * DT_IDENT_INTS;
    const int *ta = p.gt_tab + (long long)clip * acap * 2;
    const int *tb = p.hyp_tab + (long long)clip * bcap * 2;
    const long long *al = p.align + (long long)clip * acap * bcap;
    const int na = min(max(sz[3], 0), acap), nb = min(max(sz[4], 0), bcap);
    const int ng = min(max(p.gt_counts[frame], 0), gcap), nh = min(max(p.hyp_counts[frame], 0), hcap);

    for (int e = lane; e < na; e += 64) {
        const int2 r = *reinterpret_cast<const int2 *>(ta + (long long)e * 2);
        a_id[e] = r.x; a_n[e] = r.y;
    }
    for (int e = lane; e < nb; e += 64) {
        const int2 r = *reinterpret_cast<const int2 *>(tb + (long long)e * 2);
        b_id[e] = r.x; b_n[e] = r.y;
    }
    hota_load_rows(p.gt_boxes + frame * gcap * DT_BOX_FLOATS, p.gt_ids + frame * gcap, ng, 1, 5, gx, gy, gw, gh, gl, g_id, lane);
    hota_load_rows(p.hyp_boxes + frame * hcap * 8, p.hyp_ids + frame * hcap * p.id_stride, nh, p.id_stride, p.label_at, hx, hy, hw, hh, hl, h_id,
                   lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    find_trajectories(g_id, g_ent, ng, a_id, na, lane);
    find_trajectories(h_id, h_ent, nh, b_id, nb, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();

    if (lane == 0) *reinterpret_cast<int2 *>(p.dims + frame * 2) = make_int2(ng, nh);
    for (int g = lane; g < gcap; g += 64) p.gt_ent[frame * gcap + g] = g < ng ? g_ent[g] : -1;
    for (int i = lane; i < hcap; i += 64) p.hyp_ent[frame * hcap + i] = i < nh ? h_ent[i] : -1;
    int *w = p.w + frame * gcap * hcap;
    for (int g = 0; g < gcap; ++g) {
        const int a = g < ng ? g_ent[g] : -1;
        int *row = w + (long long)g * hcap;
        if (a < 0) {
            for (int i = lane; i < hcap; i += 64) row[i] = 0;
            continue;
        }
        const float ax = gx[g], ay = gy[g], aw = gw[g], ah = gh[g], al_ = gl[g];
        const long long n_a = a_n[a];
        const long long *prow = al + (long long)a * bcap;
        for (int i = lane; i < hcap; i += 64) {
            int wt = 0;
            const int b = i < nh ? h_ent[i] : -1;
            if (b >= 0 && (ANY || hl[i] == al_)) {
                const int q = hota_q(bbox_iou_ref(ax, ay, aw, ah, hx[i], hy[i], hw[i], hh[i]));
                if (q > 0) {
                    const long long P = prow[b];
                    // P <= 2^20 * min(n_a, n_b): the divisor is >= 2^20 * max(n_a, n_b) > 0 and the quotient <= q <= 2^20
                    wt = 1 + (int)((P * q) / ((long long)DT_ASSIGN_IOU_SCALE * (n_a + b_n[b]) - P));
                }
            }
            row[i] = wt;
        }
    }
}

__global__ __launch_bounds__(64) void hota_count_kernel(HotaCountArgs p)
{
    __shared__ int h_tp[DT_HOTA_MAX_THR];
    __shared__ unsigned long long h_loc[DT_HOTA_MAX_THR];
    const int clip = blockIdx.x / p.T, lane = threadIdx.x;
    const int gcap = p.gcap, hcap = p.hcap, acap = p.acap, bcap = p.bcap, n_thr = p.n_thr;
    const long long frame = blockIdx.x;
    if (lane < DT_HOTA_MAX_THR) { h_tp[lane] = 0; h_loc[lane] = 0ull; }
    __syncthreads();
    const int ng = min(max(p.dims[frame * 2], 0), gcap), nh = min(max(p.dims[frame * 2 + 1], 0), hcap);
    const float *gtb = p.gt_boxes + frame * gcap * DT_BOX_FLOATS;
    const float *hpb = p.hyp_boxes + frame * hcap * 8;
    int *pairs = p.pairs + (long long)clip * n_thr * acap * bcap;
    for (int g = lane; g < ng; g += 64) {
        const int i = p.row_to_col[frame * gcap + g];
        if (i < 0 || i >= nh) continue;
        const int a = p.gt_ent[frame * gcap + g], b = p.hyp_ent[frame * hcap + i];
        if (a < 0 || a >= acap || b < 0 || b >= bcap) continue;              // (a matched pair has both: its weight was not 0)
        const float4 x = *reinterpret_cast<const float4 *>(gtb + (long long)g * DT_BOX_FLOATS);
        const float4 y = *reinterpret_cast<const float4 *>(hpb + (long long)i * 8);
        const float iou = bbox_iou_ref(x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w);
        int level = 0;
        for (int k = 0; k < n_thr; ++k) level += iou >= p.thr[k] ? 1 : 0;
        if (level == 0) continue;
        atomicAdd(&h_tp[level - 1], 1);
        atomicAdd(&h_loc[level - 1], (unsigned long long)hota_q(iou));
        atomicAdd(pairs + ((long long)(level - 1) * acap + a) * bcap + b, 1);
    }
    __syncthreads();
    if (lane < n_thr && h_tp[lane] != 0) {
        atomicAdd(p.tp + (long long)clip * n_thr + lane, h_tp[lane]);
        atomicAdd(reinterpret_cast<unsigned long long *>(p.loc + (long long)clip * n_thr + lane), h_loc[lane]);
    }
}

size_t hota_align_lds_bytes(int gcap, int hcap, int acap, int bcap)
{
    return ((size_t)2 * (size_t)acap + (size_t)2 * (size_t)bcap + (size_t)9 * (size_t)gcap + (size_t)9 * (size_t)hcap) * sizeof(int);
}

size_t hota_weights_lds_bytes(int gcap, int hcap, int acap, int bcap)
{
    return ((size_t)2 * (size_t)acap + (size_t)2 * (size_t)bcap + (size_t)7 * (size_t)gcap + (size_t)7 * (size_t)hcap) * sizeof(int);
}

template <typename K>
static int hota_lds_attr(PerDeviceOnce &attr, K kernel)
{
    return attr.ensure(nullptr, [kernel](int) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, HOTA_LDS_LIMIT) != hipSuccess;
    });
}

template <bool ANY>
static int launch_hota_align_as(hipStream_t st, size_t lds, const HotaArgs &a, int n_clips, int resume)
{
    static PerDeviceOnce attr;
    if (hota_lds_attr(attr, hota_align_kernel<ANY>)) return 1;
    hipLaunchKernelGGL((hota_align_kernel<ANY>), dim3((unsigned)n_clips), dim3(64), lds, st, a, resume);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// dt_hota_align (network.hip), the only caller, has validated every argument and the LDS size: nothing is checked again here
int launch_hota_align(hipStream_t st, const HotaArgs &a, int n_clips, int flags)
{
    const size_t lds = hota_align_lds_bytes(a.gcap, a.hcap, a.acap, a.bcap);
    const int resume = (flags & DT_SCORE_RESUME) ? 1 : 0;
    if (!resume && hipMemsetAsync(a.align, 0, (size_t)n_clips * a.acap * a.bcap * sizeof(long long), st) != hipSuccess) return 1;
    return (flags & DT_SCORE_ANY_LABEL) ? launch_hota_align_as<true>(st, lds, a, n_clips, resume)
                                        : launch_hota_align_as<false>(st, lds, a, n_clips, resume);
}

template <bool ANY>
static int launch_hota_weights_as(hipStream_t st, size_t lds, const HotaArgs &a, int n_clips)
{
    static PerDeviceOnce attr;
    if (hota_lds_attr(attr, hota_weights_kernel<ANY>)) return 1;
    hipLaunchKernelGGL((hota_weights_kernel<ANY>), dim3((unsigned)(n_clips * a.T)), dim3(64), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// dt_hota_weights has validated the arguments, n_clips * T < 2^31 among them
int launch_hota_weights(hipStream_t st, const HotaArgs &a, int n_clips, int flags)
{
    const size_t lds = hota_weights_lds_bytes(a.gcap, a.hcap, a.acap, a.bcap);
    return (flags & DT_SCORE_ANY_LABEL) ? launch_hota_weights_as<true>(st, lds, a, n_clips) : launch_hota_weights_as<false>(st, lds, a, n_clips);
}

// dt_hota_count has validated the arguments
int launch_hota_count(hipStream_t st, const HotaCountArgs &a, int n_clips, int flags)
{
    if (!(flags & DT_SCORE_RESUME)) {
        const size_t k = (size_t)n_clips * a.n_thr;
        if (hipMemsetAsync(a.tp, 0, k * sizeof(int), st) != hipSuccess || hipMemsetAsync(a.loc, 0, k * sizeof(long long), st) != hipSuccess ||
            hipMemsetAsync(a.pairs, 0, k * a.acap * a.bcap * sizeof(int), st) != hipSuccess)
            return 1;
    }
    hipLaunchKernelGGL(hota_count_kernel, dim3((unsigned)(n_clips * a.T)), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
