// score.hip -- track scoring (BUILD-DEFINED, DESIGN.md "Track scoring"): CLEAR-MOT counts of a tracker's output against
// ground-truth tracks.  One 64-lane workgroup per clip, the frames in sequence; lanes cover the hypotheses, the ground-truth
// rows and the entries of the object table in passes of 64.
//
// Per frame (all reads of the object table see it as the previous frame left it; it is written behind the match):
//   1. carry-over: ground-truth row g, ascending, whose object was last matched to track id tau >= 0 takes the lowest unclaimed
//      hypothesis of id tau if that pair is valid (IoU >= thr, equal labels unless ANY);
//   2. the rest: among the unmatched rows and unclaimed hypotheses the valid pair of the largest IoU is taken repeatedly, ties to
//      the lowest g, then the lowest i -- the best-IoU-first order of associate.hip:associate_table_kernel, in its LDS form;
//   3. counts of the frame, then the table update with the result of a walk in g order.
//
// This translation unit is compiled with -ffp-contract=off: the IoU is bbox_iou_ref's float32 bits (dt_internal.h).
// LDS, in words: 8 * ocap (the table, one array per field, and the highest row of the frame that names each entry)
//              + 11 * gcap (x, y, w, h, label, id, entry, match, IoU of the match, best key, best hypothesis)
//              + 7 * hcap (x, y, w, h, label, id, claimed).
#include "dt_internal.h"

#define SCORE_LDS_LIMIT (160 * 1024)

template <bool ANY>
__global__ __launch_bounds__(64) void track_score_kernel(ScoreArgs p, int resume)
{
    extern __shared__ __attribute__((aligned(16))) int smem_i[];
    const int clip = blockIdx.x, lane = threadIdx.x;
    const int T = p.T, gcap = p.gcap, hcap = p.hcap, ocap = p.ocap;
    const float thr = p.thr;
    // the object table: gt id, last track id, present, matched, switches, fragments, last appearance matched | scratch
    volatile int *o_gid = smem_i, *o_last = o_gid + ocap, *o_pres = o_last + ocap, *o_mat = o_pres + ocap, *o_sw = o_mat + ocap;
    volatile int *o_fr = o_sw + ocap, *o_lm = o_fr + ocap, *o_win = o_lm + ocap;
    // the frame's ground truth
    volatile float *gx = reinterpret_cast<volatile float *>(o_win + ocap), *gy = gx + gcap, *gw = gy + gcap, *gh = gw + gcap, *gl = gh + gcap;
    volatile int *g_id = reinterpret_cast<volatile int *>(gl + gcap), *g_ent = g_id + gcap, *g_m = g_ent + gcap;
    volatile float *g_iou = reinterpret_cast<volatile float *>(g_m + gcap);
    volatile unsigned *g_key = reinterpret_cast<volatile unsigned *>(g_iou + gcap);      // best remaining key; behind the match: switch | fragment << 1
    volatile int *g_best = reinterpret_cast<volatile int *>(g_key + gcap);
    // the frame's hypotheses
    volatile float *hx = reinterpret_cast<volatile float *>(g_best + gcap), *hy = hx + hcap, *hw = hy + hcap, *hh = hw + hcap, *hl = hh + hcap;
    volatile int *h_id = reinterpret_cast<volatile int *>(hl + hcap), *h_cl = h_id + hcap;

    const float *gtb = p.gt_boxes + (long long)clip * T * gcap * DT_BOX_FLOATS;
    const int *gtc = p.gt_counts + (long long)clip * T;
    const int *gti = p.gt_ids + (long long)clip * T * gcap;
    const float *hpb = p.hyp_boxes + (long long)clip * T * hcap * 8;
    const int *hpc = p.hyp_counts + (long long)clip * T;
    const int *hpi = p.hyp_ids + (long long)clip * T * hcap * p.id_stride;
    int *tot = p.totals + (long long)clip * DT_SCORE_INTS;
    int *ob = p.objs + (long long)clip * ocap * DT_SCORE_OBJ_INTS;
    int *fc = p.fcounts ? p.fcounts + (long long)clip * T * 4 : nullptr;
    int *mo = p.match ? p.match + (long long)clip * T * gcap : nullptr;
    float *io = p.match ? p.miou + (long long)clip * T * gcap : nullptr;

    int nobj = 0;
    int s_frames = 0, s_gt = 0, s_hyp = 0, s_match = 0, s_sw = 0, s_fr = 0, s_over = 0;
    if (resume) {
        s_frames = tot[0]; s_gt = tot[1]; s_hyp = tot[2]; s_match = tot[3]; s_sw = tot[4]; s_fr = tot[5]; s_over = tot[6];
        nobj = min(max(p.nobjs[clip], 0), ocap);
        for (int e = lane; e < nobj; e += 64) {
            const int4 a = *reinterpret_cast<const int4 *>(ob + (long long)e * DT_SCORE_OBJ_INTS);
            const int4 b = *reinterpret_cast<const int4 *>(ob + (long long)e * DT_SCORE_OBJ_INTS + 4);
            o_gid[e] = a.x; o_last[e] = a.y; o_pres[e] = a.z; o_mat[e] = a.w; o_sw[e] = b.x; o_fr[e] = b.y; o_lm[e] = b.z;
        }
    }
    for (int t = 0; t < T; ++t) {
        const int ng = min(max(gtc[t], 0), gcap), nh = min(max(hpc[t], 0), hcap);
        const int nobj0 = nobj;                               // the table as the previous frame left it
        for (int g = lane; g < ng; g += 64) {
            const float *q = gtb + ((long long)t * gcap + g) * DT_BOX_FLOATS;
            const float4 b = *reinterpret_cast<const float4 *>(q);
            gx[g] = b.x; gy[g] = b.y; gw[g] = b.z; gh[g] = b.w; gl[g] = q[5];
            g_id[g] = gti[(long long)t * gcap + g];
            g_m[g] = -1; g_iou[g] = 0.0f; g_key[g] = 0u;
        }
        for (int i = lane; i < nh; i += 64) {
            const float *q = hpb + ((long long)t * hcap + i) * 8;
            const float4 b = *reinterpret_cast<const float4 *>(q);
            hx[i] = b.x; hy[i] = b.y; hw[i] = b.z; hh[i] = b.w; hl[i] = q[p.label_at];
            h_id[i] = hpi[((long long)t * hcap + i) * p.id_stride];
            h_cl[i] = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // the entry of every row's object, lane = row (ids in the table are distinct; an id < 0 has no memory)
        for (int g = lane; g < ng; g += 64) {
            const int id = g_id[g];
            int e = -1;
            if (id >= 0)
                for (int k = 0; k < nobj0; ++k) e = o_gid[k] == id ? k : e;
            g_ent[g] = e;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 1. carry-over, rows in ascending order: lanes search the hypotheses for the row's last track id ----
        for (int g0 = 0; g0 < ng; g0 += 64) {
            const int g = g0 + lane;
            int tau = -1;
            if (g < ng) {
                const int e = g_ent[g];
                if (e >= 0) tau = o_last[e];
            }
            unsigned long long todo = __ballot(tau >= 0);
            while (todo) {
                const int b = __ffsll((long long)todo) - 1, gg = g0 + b;
                const int tv = __shfl(tau, b);
                int fi = -1;
                for (int i0 = 0; i0 < nh; i0 += 64) {
                    const int i = i0 + lane;
                    const unsigned long long bal = __ballot(i < nh && h_cl[i] == 0 && h_id[i] == tv);
                    if (bal) {
                        fi = i0 + __ffsll((long long)bal) - 1;
                        break;
                    }
                }
                if (fi >= 0) {
                    const float iou = bbox_iou_ref(gx[gg], gy[gg], gw[gg], gh[gg], hx[fi], hy[fi], hw[fi], hh[fi]);
                    const bool valid = iou >= thr && (ANY || gl[gg] == hl[fi]);
                    if (valid && lane == 0) { h_cl[fi] = 1; g_m[gg] = fi; g_iou[gg] = iou; }
                }
                __builtin_amdgcn_wave_barrier();
                todo &= todo - 1ull;
            }
        }
        // ---- 2. the rest, best IoU first (associate_table_kernel's LDS form: cached best candidate per row, rounds) ----
        auto scan = [&](int g) {
            const float ax = gx[g], ay = gy[g], aw = gw[g], ah = gh[g], al = gl[g];
            unsigned bestk = 0u;
            int bj = 0;
            for (int i0 = 0; i0 < nh; i0 += 64) {
                const int i = i0 + lane;
                unsigned key = 0u;
                if (i < nh && h_cl[i] == 0 && (ANY || hl[i] == al)) {
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, hx[i], hy[i], hw[i], hh[i]);
                    if (iou >= thr) key = __float_as_uint(iou) + 1u;
                }
                const unsigned m = wave_umax_dpp(key);
                if (m > bestk) {
                    bestk = m;
                    bj = i0 + __ffsll((long long)__ballot(key == m)) - 1;
                }
            }
            if (lane == 0) { g_key[g] = bestk; g_best[g] = bj; }
        };
        for (int g = 0; g < ng; ++g)
            if (g_m[g] < 0) scan(g);
        __builtin_amdgcn_wave_barrier();
        for (;;) {
            unsigned bestk = 0u;
            int bi = 0;
            for (int g0 = 0; g0 < ng; g0 += 64) {
                const int g = g0 + lane;
                const unsigned key = g < ng ? g_key[g] : 0u;
                const unsigned m = wave_umax_dpp(key);
                if (m > bestk) {
                    bestk = m;
                    bi = g0 + __ffsll((long long)__ballot(key == m)) - 1;
                }
            }
            if (bestk == 0u) break;
            const int bj = g_best[bi];
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {
                h_cl[bj] = 1;
                g_m[bi] = bj; g_iou[bi] = __uint_as_float(bestk - 1u); g_key[bi] = 0u;
            }
            __builtin_amdgcn_wave_barrier();
            for (int g0 = 0; g0 < ng; g0 += 64) {
                const int g = g0 + lane;
                unsigned long long again = __ballot(g < ng && g_key[g] != 0u && g_best[g] == bj);
                while (again) {
                    scan(g0 + __ffsll((long long)again) - 1);
                    again &= again - 1ull;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- 3. counts of the frame against the table as it was; per-row outputs ----
        int f_match = 0, f_sw = 0, f_fr = 0;
        for (int g0 = 0; g0 < gcap; g0 += 64) {
            const int g = g0 + lane;
            const int m = g < ng ? g_m[g] : -1;
            bool sw = false, fr = false;
            if (m >= 0) {
                const int e = g_ent[g];
                if (e >= 0) {
                    const int tau = o_last[e];
                    sw = tau >= 0 && tau != h_id[m];
                    fr = o_mat[e] > 0 && o_lm[e] == 0;
                }
            }
            if (g < ng) g_key[g] = (sw ? 1u : 0u) | (fr ? 2u : 0u);
            if (mo && g < gcap) {
                mo[(long long)t * gcap + g] = m;
                io[(long long)t * gcap + g] = g < ng ? g_iou[g] : 0.0f;
            }
            f_match += __popcll(__ballot(m >= 0));
            f_sw += __popcll(__ballot(sw));
            f_fr += __popcll(__ballot(fr));
        }
        if (fc && lane == 0) *reinterpret_cast<int4 *>(fc + (long long)t * 4) = make_int4(ng, nh, f_match, f_sw);
        __builtin_amdgcn_wave_barrier();
        // ---- 4. objects seen for the first time get their entries, in row order; a full table counts the box as overflow ----
        for (int g0 = 0; g0 < ng; g0 += 64) {
            const int g = g0 + lane;
            unsigned long long fresh = __ballot(g < ng && g_ent[g] < 0 && g_id[g] >= 0);
            while (fresh) {
                const int gg = g0 + __ffsll((long long)fresh) - 1;
                const int v = g_id[gg];
                int found = -1;                               // a lower row of this frame may have opened the entry
                for (int k0 = nobj0; k0 < nobj; k0 += 64) {
                    const int k = k0 + lane;
                    const unsigned long long bal = __ballot(k < nobj && o_gid[k] == v);
                    if (bal) {
                        found = k0 + __ffsll((long long)bal) - 1;
                        break;
                    }
                }
                if (found < 0) {
                    if (nobj < ocap) {
                        found = nobj++;
                        if (lane == 0) {
                            o_gid[found] = v; o_last[found] = -1; o_pres[found] = 0; o_mat[found] = 0; o_sw[found] = 0; o_fr[found] = 0;
                            o_lm[found] = 0;
                        }
                    } else {
                        ++s_over;
                    }
                }
                if (found >= 0 && lane == 0) g_ent[gg] = found;
                __builtin_amdgcn_wave_barrier();
                fresh &= fresh - 1ull;
            }
        }
        // ---- 5. the update, with the result of the walk in row order.  An id may occur in several rows of a frame: the counters add
        //         (LDS atomics, order-free); the highest such row sets last-appearance-matched and the highest MATCHED one the last
        //         track id -- what the last writer of each field leaves -- both found by an atomic max per entry.  The entry's
        //         last-appearance word was consumed by the counts above and holds the second maximum until it is rewritten ----
        for (int g = lane; g < ng; g += 64) {
            const int e = g_ent[g];
            if (e >= 0) { o_win[e] = -1; o_lm[e] = -1; }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int g = lane; g < ng; g += 64) {
            const int e = g_ent[g];
            if (e < 0) continue;
            atomicMax(const_cast<int *>(o_win + e), g);
            if (g_m[g] >= 0) atomicMax(const_cast<int *>(o_lm + e), g);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int g = lane; g < ng; g += 64) {
            const int e = g_ent[g];
            if (e < 0) continue;
            const int m = g_m[g];
            const unsigned f = g_key[g];
            atomicAdd(const_cast<int *>(o_pres + e), 1);
            if (m >= 0) atomicAdd(const_cast<int *>(o_mat + e), 1);
            if (f & 1u) atomicAdd(const_cast<int *>(o_sw + e), 1);
            if (f & 2u) atomicAdd(const_cast<int *>(o_fr + e), 1);
            g_key[g] = f | (o_win[e] == g ? 4u : 0u) | (m >= 0 && o_lm[e] == g ? 8u : 0u);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int g = lane; g < ng; g += 64) {
            const int e = g_ent[g];
            if (e < 0) continue;
            const int m = g_m[g];
            const unsigned f = g_key[g];
            if (f & 4u) o_lm[e] = m >= 0 ? 1 : 0;
            if (f & 8u) o_last[e] = h_id[m];
        }
        s_frames += 1; s_gt += ng; s_hyp += nh; s_match += f_match; s_sw += f_sw; s_fr += f_fr;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) {
        *reinterpret_cast<int4 *>(tot) = make_int4(s_frames, s_gt, s_hyp, s_match);
        *reinterpret_cast<int4 *>(tot + 4) = make_int4(s_sw, s_fr, s_over, 0);
        p.nobjs[clip] = nobj;
    }
    for (int e = lane; e < ocap; e += 64) {
        const bool in = e < nobj;
        *reinterpret_cast<int4 *>(ob + (long long)e * DT_SCORE_OBJ_INTS) =
            in ? make_int4(o_gid[e], o_last[e], o_pres[e], o_mat[e]) : make_int4(-1, -1, 0, 0);
        *reinterpret_cast<int4 *>(ob + (long long)e * DT_SCORE_OBJ_INTS + 4) = in ? make_int4(o_sw[e], o_fr[e], o_lm[e], 0) : make_int4(0, 0, 0, 0);
    }
}

size_t track_score_lds_bytes(int gcap, int hcap, int ocap)
{
    return ((size_t)8 * (size_t)ocap + (size_t)11 * (size_t)gcap + (size_t)7 * (size_t)hcap) * sizeof(int);
}

template <bool ANY>
static int launch_track_score_as(hipStream_t st, size_t lds, const ScoreArgs &a, int n_clips, int resume)
{
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(track_score_kernel<ANY>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       SCORE_LDS_LIMIT) != hipSuccess;
        }))
        return 1;
    hipLaunchKernelGGL((track_score_kernel<ANY>), dim3((unsigned)n_clips), dim3(64), lds, st, a, resume);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// dt_track_score (network.hip), the only caller, has validated every argument and the LDS size: nothing is checked again here
int launch_track_score(hipStream_t st, const ScoreArgs &a, int n_clips, int flags)
{
    const size_t lds = track_score_lds_bytes(a.gcap, a.hcap, a.ocap);
    const int resume = (flags & DT_SCORE_RESUME) ? 1 : 0;
    return (flags & DT_SCORE_ANY_LABEL) ? launch_track_score_as<true>(st, lds, a, n_clips, resume)
                                        : launch_track_score_as<false>(st, lds, a, n_clips, resume);
}
