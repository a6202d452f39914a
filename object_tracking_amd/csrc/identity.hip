// identity.hip -- identity scoring (BUILD-DEFINED, DESIGN.md "Identity scoring"): the overlap of ground-truth trajectories with
// hypothesis trajectories over a clip, and an exact integer maximum-weight assignment.  IDTP is the assignment's total on the overlap;
// IDF1 and its siblings are ratios of integers, taken on the host.  Both kernels run one 64-lane workgroup per clip / problem.
//
// identity_overlap_kernel, per frame:
//   1. every row finds the table row of its id (lane = row, the table walked once); ids seen for the first time are appended in row
//      order by a serial loop over the new rows only (track_score_kernel's step 4), for the ground truth and for the hypotheses alike;
//      a full table counts the box as overflow; the boxes of a trajectory are counted with LDS atomic adds (an id may repeat in a frame);
//   2. lanes cover the hypotheses of ground-truth row g: a valid pair (IoU >= thr, equal labels unless ANY) whose rows both have a
//      trajectory adds 1 to overlap[a][b] in global memory.  Nothing is claimed: every valid pair of the frame counts.
// This translation unit is compiled with -ffp-contract=off: the IoU is bbox_iou_ref's float32 bits (dt_internal.h).
// LDS, in words: 2 * acap + 2 * bcap (id and boxes of every trajectory) + 7 * gcap + 7 * hcap (x, y, w, h, label, id, trajectory).
//
// assign_max_kernel: the shortest-augmenting-path Hungarian method with integer potentials on the costs c = -w, on the orientation
// whose row count is the smaller (the matrix's own rows on a tie), transposed by index only.  Rows and columns of the solve are counted
// from 1; column 0 is the method's root.  With 0 <= w <= 2^24 = C every potential stays in [-C, 0] and every reduced cost in
// [-C, 2C], so int32 is exact; the arithmetic is done on unsigned words so that weights outside the contract wrap
// instead of overflowing, and every loop is counted, so such a call still ends and stays in bounds.
// LDS, in words: 6 * (max(rcap, ccap) + 1): u, v, minv, way, p, used.
#include "dt_internal.h"

#define IDENT_LDS_LIMIT (160 * 1024)

template <bool ANY>
__global__ __launch_bounds__(64) void identity_overlap_kernel(IdentArgs p, int resume)
{
    extern __shared__ __attribute__((aligned(16))) int smem_i[];
    const int clip = blockIdx.x, lane = threadIdx.x;
    const int T = p.T, gcap = p.gcap, hcap = p.hcap, acap = p.acap, bcap = p.bcap;
    const float thr = p.thr;
    // the two trajectory tables: id, boxes
    volatile int *a_id = smem_i, *a_n = a_id + acap, *b_id = a_n + acap, *b_n = b_id + bcap;
    // the frame's ground truth, then its hypotheses
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
    int *ov = p.overlap + (long long)clip * acap * bcap;      // zero (the launcher's memset), or as the previous chunk left it

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
        for (int g = lane; g < ng; g += 64) {
            const float *q = gtb + ((long long)t * gcap + g) * DT_BOX_FLOATS;
            const float4 b = *reinterpret_cast<const float4 *>(q);
            gx[g] = b.x; gy[g] = b.y; gw[g] = b.z; gh[g] = b.w; gl[g] = q[5];
            g_id[g] = gti[(long long)t * gcap + g];
        }
        for (int i = lane; i < nh; i += 64) {
            const float *q = hpb + ((long long)t * hcap + i) * 8;
            const float4 b = *reinterpret_cast<const float4 *>(q);
            hx[i] = b.x; hy[i] = b.y; hw[i] = b.z; hh[i] = b.w; hl[i] = q[p.label_at];
            h_id[i] = hpi[((long long)t * hcap + i) * p.id_stride];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // ---- 1. the trajectory of every row ----
        s_over_a += open_trajectories(g_id, g_ent, ng, a_id, a_n, na, acap, lane);
        s_over_b += open_trajectories(h_id, h_ent, nh, b_id, b_n, nb, bcap, lane);
        // ---- 2. the valid pairs, lanes over the hypotheses of row g ----
        for (int g = 0; g < ng; ++g) {
            const int a = g_ent[g];
            if (a < 0) continue;
            const float ax = gx[g], ay = gy[g], aw = gw[g], ah = gh[g], al = gl[g];
            int *row = ov + (long long)a * bcap;
            for (int i0 = 0; i0 < nh; i0 += 64) {
                const int i = i0 + lane;
                int b = -1;
                bool valid = false;
                if (i < nh) {
                    b = h_ent[i];
                    if (b >= 0 && (ANY || hl[i] == al)) valid = bbox_iou_ref(ax, ay, aw, ah, hx[i], hy[i], hw[i], hh[i]) >= thr;
                }
                if (valid) atomicAdd(row + b, 1);             // repeated ids can make two pairs hit one word
                s_pairs += __popcll(__ballot(valid));
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

size_t identity_overlap_lds_bytes(int gcap, int hcap, int acap, int bcap)
{
    return ((size_t)2 * (size_t)acap + (size_t)2 * (size_t)bcap + (size_t)7 * (size_t)gcap + (size_t)7 * (size_t)hcap) * sizeof(int);
}

template <bool ANY>
static int launch_identity_overlap_as(hipStream_t st, size_t lds, const IdentArgs &a, int n_clips, int resume)
{
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(identity_overlap_kernel<ANY>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       IDENT_LDS_LIMIT) != hipSuccess;
        }))
        return 1;
    hipLaunchKernelGGL((identity_overlap_kernel<ANY>), dim3((unsigned)n_clips), dim3(64), lds, st, a, resume);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// dt_identity_overlap (network.hip), the only caller, has validated every argument and the LDS size: nothing is checked again here
int launch_identity_overlap(hipStream_t st, const IdentArgs &a, int n_clips, int flags)
{
    const size_t lds = identity_overlap_lds_bytes(a.gcap, a.hcap, a.acap, a.bcap);
    const int resume = (flags & DT_SCORE_RESUME) ? 1 : 0;
    if (!resume && hipMemsetAsync(a.overlap, 0, (size_t)n_clips * a.acap * a.bcap * sizeof(int), st) != hipSuccess) return 1;
    return (flags & DT_SCORE_ANY_LABEL) ? launch_identity_overlap_as<true>(st, lds, a, n_clips, resume)
                                        : launch_identity_overlap_as<false>(st, lds, a, n_clips, resume);
}

// ---------------------------------------------------------------------------------------------------------------- assignment

__global__ __launch_bounds__(64) void assign_max_kernel(AssignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int smem_i[];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int rcap = a.rcap, ccap = a.ccap;
    const int L = max(rcap, ccap) + 1;
    volatile unsigned *u = reinterpret_cast<volatile unsigned *>(smem_i), *v = u + L, *minv = v + L;      // potentials and reduced costs, int32 bits
    volatile int *way = smem_i + 3 * L, *p = way + L, *used = p + L;

    const int *w = a.w + (long long)k * rcap * ccap;
    const int rows = min(max(a.dims[(long long)k * a.stride + a.rows_at], 0), rcap);
    const int cols = min(max(a.dims[(long long)k * a.stride + a.cols_at], 0), ccap);
    const bool tr = cols < rows;                              // the solve's rows are the matrix's columns
    const int N = tr ? cols : rows, M = tr ? rows : cols;
    // the weight of solve row i, solve column j (both from 1)
    auto weight = [&](int i, int j) { return tr ? w[(long long)(j - 1) * ccap + (i - 1)] : w[(long long)(i - 1) * ccap + (j - 1)]; };

    for (int j = lane; j <= M; j += 64) { v[j] = 0u; p[j] = 0; way[j] = 0; }
    for (int i = lane; i <= N; i += 64) u[i] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int i = 1; i <= N; ++i) {
        for (int j = lane; j <= M; j += 64) { minv[j] = (unsigned)ASSIGN_INF; used[j] = 0; }
        if (lane == 0) p[0] = i;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        int j0 = 0;
        for (int step = 0; step <= M; ++step) {               // at most i steps reach a free column; the bound is the algorithm's
            if (lane == 0) used[j0] = 1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            const int i0 = p[j0];
            const unsigned ui = u[i0];
            // the row's reduced costs against minv; the minimum over the unused columns and its lowest column
            unsigned bestk = 0u;
            int j1 = -1;
            for (int jb = 1; jb <= M; jb += 64) {
                const int j = jb + lane;
                const bool act = j <= M && used[j] == 0;
                unsigned key = 0u;
                if (act) {
                    const unsigned cur = 0u - (unsigned)weight(i0, j) - ui - v[j];
                    unsigned m = minv[j];
                    if ((int)cur < (int)m) { m = cur; minv[j] = cur; way[j] = j0; }
                    key = (unsigned)ASSIGN_INF - m;           // the smallest minv has the largest key; in the contract never 0
                }
                const unsigned top = wave_umax_dpp(key);
                if (top > bestk || j1 < 0) {
                    const unsigned long long bal = __ballot(act && key == top);
                    if (bal) {
                        bestk = top;
                        j1 = jb + __ffsll((long long)bal) - 1;
                    }
                }
            }
            if (j1 < 0) break;                                // no unused column: cannot happen while N <= M
            const unsigned delta = (unsigned)ASSIGN_INF - bestk;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            for (int j = lane; j <= M; j += 64) {
                if (used[j]) {                                // p is one-to-one on the used columns
                    const int pj = p[j];
                    u[pj] = u[pj] + delta;
                    v[j] = v[j] - delta;
                } else {
                    minv[j] = minv[j] - delta;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            j0 = j1;
            if (p[j0] == 0) break;
        }
        // flip the path back to the root
        if (lane == 0) {
            int j = j0;
            for (int step = 0; step <= M && j != 0; ++step) {
                const int jp = way[j];
                p[j] = p[jp];
                j = jp;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    // the result, built in LDS (minv and way are free now) so that every output word is stored once
    volatile int *r2c = reinterpret_cast<volatile int *>(minv), *c2r = way;
    for (int r = lane; r < rcap; r += 64) r2c[r] = -1;
    for (int c = lane; c < ccap; c += 64) c2r[c] = -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    long long sum = 0;
    for (int j = 1 + lane; j <= M; j += 64) {
        const int i = p[j];
        if (i < 1 || i > N) continue;
        const int wt = weight(i, j);
        if (wt == 0) continue;                                // a pair without weight is reported as unassigned
        const int r = tr ? j - 1 : i - 1, c = tr ? i - 1 : j - 1;
        r2c[r] = c; c2r[c] = r;
        sum += wt;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s);
    for (int r = lane; r < rcap; r += 64) a.row_to_col[(long long)k * rcap + r] = r2c[r];
    for (int c = lane; c < ccap; c += 64) a.col_to_row[(long long)k * ccap + c] = c2r[c];
    if (lane == 0) a.total[k] = sum;
}

size_t assign_max_lds_bytes(int rcap, int ccap)
{
    return (size_t)6 * ((size_t)(rcap > ccap ? rcap : ccap) + 1) * sizeof(int);
}

// dt_assign_max (network.hip), the only caller, has validated every argument and the LDS size
int launch_assign_max(hipStream_t st, const AssignArgs &a, int n)
{
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(assign_max_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       IDENT_LDS_LIMIT) != hipSuccess;
        }))
        return 1;
    hipLaunchKernelGGL(assign_max_kernel, dim3((unsigned)n), dim3(64), assign_max_lds_bytes(a.rcap, a.ccap), st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
