// decode.hip -- YOLO output-grid decode + per-class greedy NMS + final filter,
// and the build-defined track-ID association.  One workgroup per frame.
//
// Follows utility/utils.py:208-257 (decode_netout) with sigmoid :259, the
// GLOBAL-max/min softmax :262-270, bbox_iou :155-173, interval_overlap :175-188
// and BoundBox.get_label/get_score :128-136 (post-NMS argmax).
//
// This translation unit is compiled with -ffp-contract=off: the reference's
// numpy float32 arithmetic rounds after every multiply and add, so no fused
// multiply-add may be formed in the IoU / box math.
//
// HBM/latency-bound integer+float bookkeeping: the netout frame is staged
// through LDS in coalesced chunks ([cells][5+C] rows; the odd row length keeps
// the per-cell reads bank-conflict-free), the candidate list is compacted with
// wavefront ballots, NMS runs one class per wavefront with the suppression
// sweep spread over the 64 lanes.
#include "dt_internal.h"

#define DEC_THREADS 1024           // 16 waves: the frame is read with few bytes in flight per thread, so more threads = shorter passes
#define DEC_MAX_CELLS 1920        // 19*19*5 = 1805 fits; (5+16)*mc*4 B of LDS must stay under 160 KiB.  Larger grids (up to
#define DEC_BIG_MAX_CELLS 8192    // 8192 cells: the 13-bit cell field of the kept-score keys) run the BIG instance of the kernel, whose
                                  // per-candidate arrays and overflow sort lists live in a global scratch instead of LDS
#define DEC_CELL_BITS 13
#define DEC_CHUNK_BYTES (96 * 1024)
#define DEC_NZ_CAP 4096           // kept (cell, class) scores held in LDS for the NMS (8 B each + 16 B of sort lists)

__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf(-x)); }

// interval_overlap_ref / bbox_iou_ref (utils.py:175-188, :155-173) and wave_umax_dpp: dt_internal.h, shared with score.hip

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// block-wide exclusive prefix of a 0/1 flag, in thread order; returns prefix and total
__device__ __forceinline__ int block_flag_scan(bool flag, int *s_wave_tot /*[DEC_THREADS / 64]*/, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    const int within = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < DEC_THREADS / 64; ++w) {
        const int t = s_wave_tot[w];
        if (w < wave) base += t;
        total += t;
    }
    return base + within;
}

struct DecodeArgs {
    const float *netout;
    long long frame_stride;
    int GH, GW, NB, NC;
    float obj_thr, nms_thr;
    const float *frame_thr;   // optional [batch][2] (obj, nms) per frame: one threshold pair per camera / stream
    const float *anchors;
    int cap;
    float *boxes;
    int *counts;
    float *classes;
    float *post;        // [batch][ncell][S] (user buffer or internal scratch)
    int chunk_cells;
    int nms_waves;      // wavefronts that run the per-class NMS (each needs 4 x mc floats of LDS)
    int mc;             // ncell rounded up to 64: stride of the LDS candidate / sort arrays
    int ncp;            // NC rounded up to 4: per-class candidate counters in LDS
    int nzcap;          // capacity of the LDS list of non-zero (cell, class) scores; more than that: NMS gathers from global memory
    float *scratch;     // BIG instance: per frame [7][mc] candidate arrays | [2 mc] keys (u64) | [nms_waves][4][mc] overflow lists
    long long scratch_stride;   // floats per frame
};

// BIG = false: every per-candidate array in LDS (grids up to DEC_MAX_CELLS cells; the production sizes).  BIG = true: the
// same algorithm with the [mc]-sized arrays in a global scratch region of the frame (read and written by this workgroup
// only, ordered by its barriers) -- slower, but any grid up to DEC_BIG_MAX_CELLS cells decodes (utils.py:208-257 has no size limit).
template <bool BIG>
__global__ __launch_bounds__(DEC_THREADS) void decode_nms_kernel(DecodeArgs p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int S = 5 + p.NC;
    const int ncell = p.GH * p.GW * p.NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frame = blockIdx.x;
    const float obj_thr = p.frame_thr ? p.frame_thr[2 * frame] : p.obj_thr;
    const float nms_thr = p.frame_thr ? p.frame_thr[2 * frame + 1] : p.nms_thr;
    const float *net = p.netout + (long long)frame * p.frame_stride;
    float *post = p.post + (long long)frame * ncell * S;

    // LDS carve: candidate arrays first (persistent), then a region that is the staging chunk in phase 2 and the
    // per-class sort lists in phase 3.
    const int MC = p.mc;
    float *const cand = BIG ? p.scratch + (long long)frame * p.scratch_stride : smem;   // [7][MC] candidate arrays
    int *s_cell = reinterpret_cast<int *>(cand);              // [MC] cell of candidate k
    float *s_bx = cand + MC;                                  // [4][MC] box of candidate k
    int *s_kof = reinterpret_cast<int *>(cand + 5 * MC);      // [MC] per cell: 'any class kept' flag, then its candidate index
    float *s_conf = cand + 6 * MC;                            // [MC] objectness of candidate k
    float *s_red = BIG ? smem : smem + 7 * MC;                // [32]: per-wave max, per-wave min
    int *s_tot = reinterpret_cast<int *>(s_red + 32);         // [16]
    int *s_nzn = reinterpret_cast<int *>(s_red + 48);         // [0]: number of non-zero (cell, class) scores
    int *s_ccnt = reinterpret_cast<int *>(s_red + 64);        // [ncp] candidates with a non-zero score per class
    int *s_coff = s_ccnt + p.ncp;                             // [ncp] start of the class's segment in the sort lists
    int *s_cfill = s_coff + p.ncp;                            // [ncp]
    float *s_sum = s_red + 64 + 3 * p.ncp;                    // [DEC_THREADS] softmax denominators of the chunk's cells
    unsigned *s_nzk = reinterpret_cast<unsigned *>(s_sum + DEC_THREADS);   // [nzcap] cell | class << DEC_CELL_BITS
    float *s_nzs = reinterpret_cast<float *>(s_nzk + p.nzcap);             // [nzcap] score
    float *s_dyn = s_nzs + p.nzcap;                           // chunk / sort lists
    // [MC] per candidate: max over its classes of (score bits << 32 | ~class) after the NMS; takes the place of the
    // (cell, class, score) list once that has been bucketed (8 nzcap >= 8 MC bytes: launch_decode)
    unsigned long long *s_key = BIG ? reinterpret_cast<unsigned long long *>(cand + 7 * MC) : reinterpret_cast<unsigned long long *>(s_nzk);

    // ---- phase 1: global max / min of the class logits (utils.py:263-264) ----
    float vmax = -INFINITY, vmin = INFINITY;
    const int nelem = ncell * S;
    for (int c = tid; c < p.ncp; c += DEC_THREADS) { s_ccnt[c] = 0; s_cfill[c] = 0; }
    if (tid == 0) s_nzn[0] = 0;
    // 16-byte loads (a CU streams dword loads at ~12 B/clk only): frames are 4-byte aligned, so up to three leading
    // elements (channels 0..2 of cell 0: never class logits) and up to three trailing ones are taken apart
    const int head = (4 - (int)((reinterpret_cast<uintptr_t>(net) >> 2) & 3)) & 3;
    {
        // channel of element e is e % S; advance it incrementally and keep eight independent loads in flight
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 *vp = reinterpret_cast<const f4 *>(net + head);
        const int nvec = (nelem - head) >> 2;
        const int step = (4 * DEC_THREADS) % S;
        int ch = (head + 4 * tid) % S;
        auto upd4 = [&](const f4 &v, int c0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int c = c0 + q;
                if (c >= S) c -= S;
                if (c >= 5) { vmax = fmaxf(vmax, v[q]); vmin = fminf(vmin, v[q]); }
            }
        };
        int i = tid;
        for (; i + 7 * DEC_THREADS < nvec; i += 8 * DEC_THREADS) {
            f4 v[8];
            int c8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[u] = vp[i + u * DEC_THREADS];
                c8[u] = ch;
                ch += step;
                if (ch >= S) ch -= S;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) upd4(v[u], c8[u]);
        }
        for (; i < nvec; i += DEC_THREADS) {
            upd4(vp[i], ch);
            ch += step;
            if (ch >= S) ch -= S;
        }
        const int e = head + 4 * nvec + tid;      // up to three trailing elements
        if (e < nelem && e % S >= 5) { const float v = net[e]; vmax = fmaxf(vmax, v); vmin = fminf(vmin, v); }
    }
    vmax = wave_max(vmax);
    vmin = wave_min(vmin);
    if (lane == 0) { s_red[wave] = vmax; s_red[16 + wave] = vmin; }
    __syncthreads();
    float gmax = s_red[0], gmn = s_red[16];
#pragma unroll
    for (int w = 1; w < DEC_THREADS / 64; ++w) { gmax = fmaxf(gmax, s_red[w]); gmn = fminf(gmn, s_red[16 + w]); }
    const float gmin = gmn - gmax;  // min(x - max)
    const bool rescale = gmin < -100.0f;   // utils.py:265-266

    // ---- phase 2: conf / class scores / threshold, candidate boxes -----------
    // Per staged chunk: (a) exp / sigmoid element-parallel, (b) the softmax denominator per cell, summed in class
    // order like the reference's row sum, (c) conf * (e / sum) and the threshold element-parallel -- kept scores also
    // go to the LDS list the NMS reads -- (d) one thread per cell: box of a cell with any kept class, compaction.
    int ncand = 0;
    float *const cbuf = s_dyn + ((4 - head) & 3);   // element `head` of a chunk -- 16-byte aligned in global memory -- is 16-byte aligned in LDS too
    const unsigned c_magic = 0xFFFFFFFFu / (unsigned)p.NC + 1u;   // e2 / NC == umulhi(e2, magic) for e2 * NC < 2^32 (chunk elements < 2^15); NC == 1: identity
    for (int c0 = 0; c0 < ncell; c0 += p.chunk_cells) {
        const int cn = min(p.chunk_cells, ncell - c0);
        const int ne = cn * S;
        const float *src = net + (long long)c0 * S;
        __syncthreads();
        {   // chunk_cells is a multiple of 64, so the chunk starts at the frame's alignment
            typedef float f4 __attribute__((ext_vector_type(4)));
            const f4 *vp = reinterpret_cast<const f4 *>(src + head);
            const int nvec = (ne - head) >> 2;
            int i = tid;
            for (; i + 3 * DEC_THREADS < nvec; i += 4 * DEC_THREADS) {
                f4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = vp[i + u * DEC_THREADS];
#pragma unroll
                for (int u = 0; u < 4; ++u) *reinterpret_cast<f4 *>(cbuf + head + 4 * (i + u * DEC_THREADS)) = v[u];
            }
            for (; i < nvec; i += DEC_THREADS) {
                *reinterpret_cast<f4 *>(cbuf + head + 4 * i) = vp[i];
            }
            if (tid < head) cbuf[tid] = src[tid];
            const int e = head + 4 * nvec + tid;
            if (e < ne) cbuf[e] = src[e];
        }
        __syncthreads();
        const int nce = cn * p.NC;                               // class elements of the chunk: (cell lc, class c) <- e2 = lc * NC + c
        // (p) objectness first: conf * softmax <= conf, so a cell with conf <= threshold keeps no class whatever its
        // logits are -- its scores are written as 0 without evaluating a single exp (most cells of a frame)
        if (tid < cn) {
            float *r = cbuf + tid * S;
            const float conf = sigmoid_ref(r[4]);               // utils.py:214
            r[4] = conf;
            s_sum[tid] = conf > obj_thr ? 0.0f : -1.0f;         // < 0: no class of this cell can pass
            s_kof[c0 + tid] = 0;
        }
        __syncthreads();
        for (int e2 = tid; e2 < nce; e2 += DEC_THREADS) {       // (a)
            const int lc = p.NC == 1 ? e2 : (int)__umulhi((unsigned)e2, c_magic);
            const int e = e2 + 5 * (lc + 1);                    // lc * S + 5 + c
            float v = 0.0f;
            if (s_sum[lc] >= 0.0f) {                            // (nearly) wave-uniform: 64 lanes span one or two cells at NC = 80
                v = cbuf[e] - gmax;
                if (rescale) v = v / gmin * -100.0f;
                v = expf(v);
            }
            cbuf[e] = v;
        }
        __syncthreads();
        if (tid < cn && s_sum[tid] >= 0.0f) {                   // (b)
            const float *r = cbuf + tid * S + 5;
            float sum = 0.0f;
            int c = 0;
            for (; c + 8 <= p.NC; c += 8) {                     // reads batched, adds in class order
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = r[c + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) sum += v[u];
            }
            for (; c < p.NC; ++c) sum += r[c];
            s_sum[tid] = sum;                                   // >= 0 (or NaN, which is not < 0: the cell is still scored, like the reference)
        }
        __syncthreads();
        for (int e2 = tid; e2 < nce; e2 += DEC_THREADS) {       // (c)
            const int lc = p.NC == 1 ? e2 : (int)__umulhi((unsigned)e2, c_magic);
            const float sum = s_sum[lc];
            if (sum < 0.0f) continue;                           // its class entries are already 0
            const int c = e2 - lc * p.NC;
            const int e = e2 + 5 * (lc + 1);
            const float pr = cbuf[lc * S + 4] * (cbuf[e] / sum);           // :215
            const float keep = pr > obj_thr ? pr : 0.0f;                   // :216
            cbuf[e] = keep;
            if (keep != 0.0f) {
                s_kof[c0 + lc] = 1;
                atomicAdd(&s_ccnt[c], 1);
                const int at = atomicAdd(&s_nzn[0], 1);
                if (at < p.nzcap) { s_nzk[at] = (unsigned)(c0 + lc) | ((unsigned)c << DEC_CELL_BITS); s_nzs[at] = keep; }
            }
        }
        __syncthreads();
        {                                                       // (d): chunk_cells <= DEC_THREADS
            const int lc = tid;
            const bool any = lc < cn && s_kof[c0 + lc] != 0;
            float bx = 0, by = 0, bw = 0, bh = 0;
            if (any) {   // :227-231
                const float *r = cbuf + lc * S;
                const int cell = c0 + lc;
                const int b = cell % p.NB;
                const int col = (cell / p.NB) % p.GW;
                const int row = cell / (p.NB * p.GW);
                bx = ((float)col + sigmoid_ref(r[0])) / (float)p.GW;
                by = ((float)row + sigmoid_ref(r[1])) / (float)p.GH;
                bw = p.anchors[2 * b + 0] * expf(r[2]) / (float)p.GW;
                bh = p.anchors[2 * b + 1] * expf(r[3]) / (float)p.GH;
            }
            int tot;
            const int slot = ncand + block_flag_scan(any, s_tot, tot);
            if (any) {
                s_cell[slot] = c0 + lc;
                s_kof[c0 + lc] = slot;
                s_conf[slot] = cbuf[lc * S + 4];
                s_bx[0 * MC + slot] = bx;
                s_bx[1 * MC + slot] = by;
                s_bx[2 * MC + slot] = bw;
                s_bx[3 * MC + slot] = bh;
            }
            ncand += tot;
        }
        {
            float *dst = post + (long long)c0 * S;
            for (int e = tid; e < ne; e += DEC_THREADS) dst[e] = cbuf[e];
        }
    }
    __syncthreads();   // post[] and candidate arrays visible to the whole workgroup

    // ---- phase 3: greedy NMS, one class per wavefront (utils.py:239-252) -----
    const int nzn = s_nzn[0];
    if (nzn <= p.nzcap) {
        // the kept (cell, class, score) triples are in LDS: bucket them by class -- each class's segment of U is its
        // unsorted list, the same segment of L its sorted list -- and let all 16 wavefronts take classes
        float *u_sc0 = s_dyn;
        int *u_id0 = reinterpret_cast<int *>(s_dyn + p.nzcap);
        float *l_sc0 = s_dyn + 2 * p.nzcap;
        int *l_id0 = reinterpret_cast<int *>(s_dyn + 3 * p.nzcap);
        if (wave == 0) {   // exclusive prefix of the per-class counts
            int running = 0;
            for (int cb = 0; cb < p.NC; cb += 64) {
                const int v = cb + lane < p.NC ? s_ccnt[cb + lane] : 0;
                int inc = v;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int t = __shfl_up(inc, o);
                    if (lane >= o) inc += t;
                }
                if (cb + lane < p.NC) s_coff[cb + lane] = running + inc - v;
                running += __builtin_amdgcn_readlane(inc, 63);
            }
        }
        __syncthreads();
        for (int i = tid; i < nzn; i += DEC_THREADS) {
            const unsigned key = s_nzk[i];
            const int c = (int)(key >> DEC_CELL_BITS);
            const int at = s_coff[c] + atomicAdd(&s_cfill[c], 1);
            u_sc0[at] = s_nzs[i];
            u_id0[at] = s_kof[key & ((1u << DEC_CELL_BITS) - 1u)];
        }
        __syncthreads();
        for (int k = tid; k < ncand; k += DEC_THREADS) s_key[k] = 0ull;
        __syncthreads();
        for (int c = wave; c < p.NC; c += DEC_THREADS / 64) {
            const int n = s_ccnt[c];
            if (n == 0) continue;   // wave-uniform
            volatile float *u_sc = u_sc0 + s_coff[c];
            volatile int *u_id = u_id0 + s_coff[c];
            volatile float *l_sc = l_sc0 + s_coff[c];
            volatile int *l_id = l_id0 + s_coff[c];
            const unsigned long long ctag = 0xFFFFFFFFull - (unsigned long long)c;   // equal scores: the lower class wins (np.argmax)
            if (n == 1) {   // nothing to suppress
                if (lane == 0) atomicMax(&s_key[u_id[0]], ((unsigned long long)__float_as_uint(u_sc[0]) << 32) | ctag);
                continue;
            }
            if (n <= 64) {
                // the whole class in one wavefront's registers: lane = list entry; rank by lane broadcasts, one LDS
                // exchange into sorted order, then the greedy sweep with the suppressed set as a wave-uniform bit mask
                const bool in = lane < n;
                const float si = in ? u_sc[lane] : 0.0f;
                const int ki = in ? u_id[lane] : -1;
                int rank = 0;
                for (int j = 0; j < n; ++j) {
                    const float sj = readlane_f(si, j);
                    const int kj = __builtin_amdgcn_readlane(ki, j);
                    rank += (sj > si || (sj == si && kj > ki)) ? 1 : 0;
                }
                if (in) { l_sc[rank] = si; l_id[rank] = ki; }
                const float sc = in ? l_sc[lane] : 0.0f;
                const int kk = in ? l_id[lane] : 0;
                const float bx = s_bx[kk], by = s_bx[MC + kk], bw = s_bx[2 * MC + kk], bh = s_bx[3 * MC + kk];
                unsigned long long dead = 0ull;
                for (int i = 0; i < n - 1; ++i) {
                    if ((dead >> i) & 1ull) continue;   // wave-uniform
                    const float ax = readlane_f(bx, i), ay = readlane_f(by, i), aw = readlane_f(bw, i), ah = readlane_f(bh, i);
                    const bool hit = in && lane > i && bbox_iou_ref(ax, ay, aw, ah, bx, by, bw, bh) >= nms_thr;
                    dead |= __ballot(hit);
                    if (hit) post[(long long)s_cell[kk] * S + 5 + c] = 0.0f;   // :252
                }
                // survivors of this class compete for their box's label (BoundBox.get_label / get_score, utils.py:128-136)
                if (in && !((dead >> lane) & 1ull)) atomicMax(&s_key[kk], ((unsigned long long)__float_as_uint(sc) << 32) | ctag);
                continue;
            }
            // rank sort: descending score, ties -> higher candidate index first (the order within U does not matter)
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                if (i < n) {
                    const float si = u_sc[i];
                    const int ki = u_id[i];
                    int rank = 0;
                    for (int j = 0; j < n; ++j) {
                        const float sj = u_sc[j];
                        const int kj = u_id[j];
                        rank += (sj > si || (sj == si && kj > ki)) ? 1 : 0;
                    }
                    l_sc[rank] = si;
                    l_id[rank] = ki;
                }
            }
            // greedy sweep: i sequential, j over lanes; l_sc[j] = 0 marks suppressed
            for (int i = 0; i < n - 1; ++i) {
                if (l_sc[i] == 0.0f) continue;   // wave-uniform
                const int ki = l_id[i];
                const float ax = s_bx[ki], ay = s_bx[MC + ki];
                const float aw = s_bx[2 * MC + ki], ah = s_bx[3 * MC + ki];
                for (int j = i + 1 + lane; j < n; j += 64) {
                    const int kj = l_id[j];
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, s_bx[kj], s_bx[MC + kj],
                                                   s_bx[2 * MC + kj], s_bx[3 * MC + kj]);
                    if (iou >= nms_thr) {
                        l_sc[j] = 0.0f;
                        post[(long long)s_cell[kj] * S + 5 + c] = 0.0f;   // :252
                    }
                }
            }
            for (int j = lane; j < n; j += 64) {   // survivors -> label keys, as above
                const float sc = l_sc[j];
                if (sc != 0.0f) atomicMax(&s_key[l_id[j]], ((unsigned long long)__float_as_uint(sc) << 32) | ctag);
            }
        }
    } else {
        // more kept scores than the LDS list holds: gather each class's scores from post[] (global memory)
        // per wavefront: sorted (score,id) list + unsorted staging list, MC entries each
        float *const ovf = BIG ? cand + 9 * MC : s_dyn;     // BIG: the lists follow the candidate arrays and keys in the scratch
        volatile float *l_sc = ovf + wave * (4 * MC);
        volatile int *l_id = reinterpret_cast<volatile int *>(ovf + wave * (4 * MC) + MC);
        volatile float *u_sc = ovf + wave * (4 * MC) + 2 * MC;
        volatile int *u_id = reinterpret_cast<volatile int *>(ovf + wave * (4 * MC) + 3 * MC);
        for (int c = wave; c < p.NC && wave < p.nms_waves; c += p.nms_waves) {
            if (s_ccnt[c] < 2) continue;   // fewer than two boxes carry this class: nothing to suppress (wave-uniform)
            // gather candidates with a non-zero score for class c
            int n = 0;
            for (int k0 = 0; k0 < ncand; k0 += 64) {
                const int k = k0 + lane;
                float sc = 0.0f;
                if (k < ncand) sc = post[(long long)s_cell[k] * S + 5 + c];
                const bool nz = sc != 0.0f;
                const unsigned long long bal = __ballot(nz);
                if (nz) {
                    const int pos = n + __popcll(bal & ((1ull << lane) - 1ull));
                    u_sc[pos] = sc;
                    u_id[pos] = k;
                }
                n += __popcll(bal);
            }
            if (n < 2) continue;
            // rank sort: descending score, ties -> higher candidate index first
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                if (i < n) {
                    const float si = u_sc[i];
                    const int ki = u_id[i];
                    int rank = 0;
                    for (int j = 0; j < n; ++j) {
                        const float sj = u_sc[j];
                        const int kj = u_id[j];
                        rank += (sj > si || (sj == si && kj > ki)) ? 1 : 0;
                    }
                    l_sc[rank] = si;
                    l_id[rank] = ki;
                }
            }
            // greedy sweep: i sequential, j over lanes; l_sc[j] = 0 marks suppressed
            for (int i = 0; i < n - 1; ++i) {
                if (l_sc[i] == 0.0f) continue;   // wave-uniform
                const int ki = l_id[i];
                const float ax = s_bx[ki], ay = s_bx[MC + ki];
                const float aw = s_bx[2 * MC + ki], ah = s_bx[3 * MC + ki];
                for (int j = i + 1 + lane; j < n; j += 64) {
                    const int kj = l_id[j];
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, s_bx[kj], s_bx[MC + kj],
                                                   s_bx[2 * MC + kj], s_bx[3 * MC + kj]);
                    if (iou >= nms_thr) {
                        l_sc[j] = 0.0f;
                        post[(long long)s_cell[kj] * S + 5 + c] = 0.0f;   // :252
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- phase 4: final filter, output in creation order (utils.py:255) ------
    int nout = 0;
    for (int k0 = 0; k0 < ncand; k0 += DEC_THREADS) {
        const int k = k0 + tid;
        bool keep = false;
        int lab = 0;
        float best = 0.0f;
        if (k < ncand && nzn <= p.nzcap) {
            const unsigned long long key = s_key[k];   // 0: every class of this box was suppressed -> score 0, label 0
            best = __uint_as_float((unsigned)(key >> 32));
            lab = key ? (int)(0xFFFFFFFFu - (unsigned)key) : 0;
            keep = best > obj_thr;
        } else if (k < ncand) {
            const float *r = post + (long long)s_cell[k] * S;
            best = r[5];
            for (int c = 1; c < p.NC; ++c) {
                const float v = r[5 + c];
                if (v > best) { best = v; lab = c; }   // np.argmax: first maximum
            }
            keep = best > obj_thr;
        }
        int tot;
        const int slot = nout + block_flag_scan(keep, s_tot, tot);
        if (keep && slot < p.cap) {
            const int cell = s_cell[k];
            float *o = p.boxes + ((long long)frame * p.cap + slot) * DT_BOX_FLOATS;
            o[0] = s_bx[k];
            o[1] = s_bx[MC + k];
            o[2] = s_bx[2 * MC + k];
            o[3] = s_bx[3 * MC + k];
            o[4] = s_conf[k];
            o[5] = (float)lab;
            o[6] = best;
            o[7] = (float)cell;
            if (p.classes != nullptr) {
                float *cl = p.classes + ((long long)frame * p.cap + slot) * p.NC;
                for (int c = 0; c < p.NC; ++c) cl[c] = post[(long long)cell * S + 5 + c];
            }
        }
        nout += tot;
    }
    if (tid == 0) p.counts[frame] = nout;
    {   // rows past the last box read as zero (callers may hand over uninitialised memory)
        const int first = min(nout, p.cap) * DT_BOX_FLOATS, total = p.cap * DT_BOX_FLOATS;
        float *o = p.boxes + (long long)frame * total;
        for (int e = first + tid; e < total; e += DEC_THREADS) o[e] = 0.0f;
    }
}

// floats of global scratch per frame the BIG instance needs (0: the grid fits the LDS-resident instance)
size_t decode_scratch_floats(int GH, int GW, int NB)
{
    const int ncell = GH * GW * NB;
    if (ncell <= DEC_MAX_CELLS) return 0;
    const size_t mc = (size_t)((ncell + 63) / 64) * 64;
    return (9 + 4 * (DEC_THREADS / 64)) * mc;      // [7][mc] candidates | [mc] u64 keys | [16 waves][4][mc] overflow lists
}

int launch_decode(hipStream_t st, const float *netout, long long frame_stride, int batch, int GH, int GW, int NB,
                  int NC, float obj_thr, float nms_thr, const float *anchors_dev, int cap, float *boxes,
                  int *counts, float *classes, float *post, const float *frame_thr, float *scratch)
{
    const int S = 5 + NC;
    const int ncell = GH * GW * NB;
    if (ncell > DEC_BIG_MAX_CELLS || batch <= 0) return 2;
    const bool big = ncell > DEC_MAX_CELLS;
    if (big && !scratch) return 2;
    const int mc = ((ncell + 63) / 64) * 64;
    const int ncp = (NC + 3) / 4 * 4;
    // LDS budget: candidate arrays [7][mc] (LDS-resident instance only), counters, softmax denominators, the list of kept
    // (cell, class, score) triples, and one region that is the staging chunk in phase 2 and the sort lists in phase 3
    const size_t fixed = (size_t)((big ? 0 : 7 * mc) + 64 + 3 * ncp + DEC_THREADS) * sizeof(float);
    int nzcap = DEC_NZ_CAP;
    while (nzcap > 256 && fixed + (size_t)nzcap * 8 + (size_t)nzcap * 16 > 160 * 1024) nzcap /= 2;
    size_t dyn = 160 * 1024 - fixed - (size_t)nzcap * 8;
    if (dyn > DEC_CHUNK_BYTES) dyn = DEC_CHUNK_BYTES;
    // LDS-resident instance: the per-candidate keys take the place of the kept-score list (8 nzcap >= 8 mc bytes)
    if (dyn < (size_t)nzcap * 16 || (!big && nzcap < mc)) return 2;
    int chunk = (int)((dyn - 16) / (S * sizeof(float)));   // up to three floats of alignment padding in front of the chunk
    chunk = (chunk / 64) * 64;
    if (chunk > DEC_THREADS) chunk = DEC_THREADS;
    if (chunk < 64) return 2;   // class count too large for the LDS staging chunk
    if ((long long)chunk * S * S >= (1ll << 32)) return 2;   // range of the kernel's multiply-high division by S
    DecodeArgs a;
    a.netout = netout; a.frame_stride = frame_stride;
    a.GH = GH; a.GW = GW; a.NB = NB; a.NC = NC;
    a.obj_thr = obj_thr; a.nms_thr = nms_thr; a.frame_thr = frame_thr; a.anchors = anchors_dev; a.cap = cap;
    a.boxes = boxes; a.counts = counts; a.classes = classes; a.post = post; a.chunk_cells = chunk;
    a.mc = mc;
    a.ncp = ncp;
    a.nzcap = nzcap;
    a.scratch = scratch;
    a.scratch_stride = (long long)decode_scratch_floats(GH, GW, NB);
    // overflow path of the NMS (more kept scores than nzcap): per-wave lists of 4 x mc floats -- in the dyn region of the
    // LDS-resident instance (as many waves as fit), in the scratch of the BIG one (all 16)
    int nms_waves = big ? DEC_THREADS / 64 : (int)(dyn / ((size_t)4 * mc * sizeof(float)));
    if (nms_waves < 1) return 2;
    a.nms_waves = nms_waves > DEC_THREADS / 64 ? DEC_THREADS / 64 : nms_waves;
    const size_t lds = fixed + (size_t)nzcap * 8 + dyn;
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(decode_nms_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
                   hipFuncSetAttribute(reinterpret_cast<const void *>(decode_nms_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess;
        }))
        return 1;
    if (lds > 160 * 1024) return 2;
    if (big) hipLaunchKernelGGL(decode_nms_kernel<true>, dim3((unsigned)batch), dim3(DEC_THREADS), lds, st, a);
    else hipLaunchKernelGGL(decode_nms_kernel<false>, dim3((unsigned)batch), dim3(DEC_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------
__global__ void bbox_iou_kernel(const float *pairs, int n, float *iou)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float *p = pairs + (long long)i * 8;
        iou[i] = bbox_iou_ref(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
    }
}

int launch_bbox_iou(hipStream_t st, const float *pairs, int n, float *iou)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(bbox_iou_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pairs, n, iou);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------
// Track identity (BUILD-DEFINED -- the reference has no association step and
// never reads `trackid`).  Specification, DESIGN.md
// "Track identity": frames in order; boxes of frame t in decode order; box i
// takes the id of the not-yet-claimed frame-(t-1) box j of the SAME label with
// the largest bbox_iou(i,j) >= thr (ties -> lowest j), else opens a new id.
// One wavefront per clip: t and i are sequential, j is spread over the lanes
// and reduced with wavefront shuffles.
// STREAM (dt_associate_stream): the clip continues the stream in slot carry.slots[clip] -- "the previous frame" of frame 0 is
// the slot's stored last frame (boxes, ids; an empty one for a fresh slot), ids continue from the slot's next free id, and the
// clip's last frame, its ids and the counter go back to the slot.  The stateless instance compiles none of it.
// ---------------------------------------------------------------------------
template <bool STREAM>
__global__ __launch_bounds__(64) void associate_kernel(const float *boxes, const int *counts, int T, int cap,
                                                       float thr, int *ids, int *nids, AssocCarry carry)
{
    // LDS: the previous and the current frame's boxes (x,y,w,h,label) and ids, so the
    // strictly sequential greedy loop runs on LDS latency, not on L2 round trips
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *pb = smem;                                   // [5][cap] previous frame (SoA)
    float *cb = pb + 5 * cap;                           // [5][cap] current frame
    volatile int *pid = reinterpret_cast<volatile int *>(cb + 5 * cap);   // [cap] previous ids (-1 once claimed)
    volatile int *cid = pid + cap;                      // [cap] current ids
    const int clip = blockIdx.x, lane = threadIdx.x;
    const float *bx = boxes + (long long)clip * T * cap * DT_BOX_FLOATS;
    const int *cnt = counts + (long long)clip * T;
    int *id = ids + (long long)clip * T * cap;
    int next_id = 0;
    int np = 0;
    // the slot's stored table, of which this kernel reads and leaves the last frame only: sb [tcap][8], si [tcap], sm = meta row
    float *sb = nullptr;
    int *si = nullptr, *sm = nullptr;
    if constexpr (STREAM) {
        const int slot = carry.slots[clip];
        sb = carry.boxes + (long long)slot * carry.tcap * DT_BOX_FLOATS;
        si = carry.ids + (long long)slot * carry.tcap;
        sm = carry.meta + slot * STREAM_META;
        np = min(sm[SM_COUNT] & SM_COUNT_MASK, cap);      // the age-0 entries lead the stored table: they are the last frame
        next_id = sm[SM_NEXT_ID];
    }
    // what both forms leave in the slot: the last frame as the caller handed it, its ids (from LDS or, register form, lane j's `outv`)
    auto store_slot = [&](const volatile int *lds_ids, int outv) {
        const int n = min(cnt[T - 1], cap);
        const float4 *src = reinterpret_cast<const float4 *>(bx + (long long)(T - 1) * cap * DT_BOX_FLOATS);
        float4 *dst = reinterpret_cast<float4 *>(sb);
        for (int q = lane; q < 2 * n; q += 64) dst[q] = src[q];
        for (int j = lane; j < n; j += 64) si[j] = lds_ids ? lds_ids[j] : outv;
        if (lane == 0) {
            sm[SM_COUNT] = n;                           // (no aged entries behind the frame: this rule keeps none)
            sm[SM_NEXT_ID] = next_id;
            const int f = sm[SM_ASSOC_FRAMES];
            sm[SM_ASSOC_FRAMES] = f > (1 << 30) ? f : f + T;
        }
    };
    // ---- register form (every frame of the clip has at most 64 boxes, T <= 64: the tracking workloads) ----
    // Lane j holds box j of the previous and of the current frame and its id in registers; box i reaches the other lanes
    // through v_readlane, the claim is a lane-select.  No LDS, no fence: the frame loop is the wavefront's own program order.
    // The next frame's boxes are requested a whole frame ahead (address selected, not the load: lanes >= n re-read box 0), and
    // a frame's ids are stored one frame late, after the wait for the boxes -- so the loop never waits for a store.
    const int cnt_l = lane < T ? min(cnt[lane], cap) : 0;
    if (T <= 64 && !__ballot(cnt_l > 64) && np <= 64) {      // (np: the stored frame sits in the same registers)
        auto request = [&](int t, float4 &q, float &ql) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float *src = bx + ((long long)t * cap + (lane < n ? lane : 0)) * DT_BOX_FLOATS;
            q = *reinterpret_cast<const float4 *>(src);
            ql = src[5];
        };
        float4 nq; float nl;
        request(0, nq, nl);
        float pbx = 0.0f, pby = 0.0f, pbw = 0.0f, pbh = 0.0f, pbl = 0.0f;
        int pidv = -1, outv = -1;
        if constexpr (STREAM) {
            if (lane < np) {
                const float *q = sb + lane * DT_BOX_FLOATS;
                const float4 v = *reinterpret_cast<const float4 *>(q);
                pbx = v.x; pby = v.y; pbw = v.z; pbh = v.w; pbl = q[5];
                pidv = si[lane];
            }
        }
        for (int t = 0; t < T; ++t) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float cx = nq.x, cy = nq.y, cw = nq.z, ch = nq.w, cl = nl;        // waits for frame t's boxes
            if (t + 1 < T) request(t + 1, nq, nl);
            if (t > 0)
                for (int j = lane; j < cap; j += 64) id[(t - 1) * cap + j] = j < 64 ? outv : -1;
            int cid = -1;
            for (int i = 0; i < n; ++i) {
                const float ax = readlane_f(cx, i), ay = readlane_f(cy, i), aw = readlane_f(cw, i), ah = readlane_f(ch, i);
                const float al = readlane_f(cl, i);
                // largest IoU among the unclaimed same-label boxes of the previous frame, ties -> lowest j (as below)
                const float iou = bbox_iou_ref(ax, ay, aw, ah, pbx, pby, pbw, pbh);
                const unsigned key = (lane < np && pidv >= 0 && pbl == al && iou >= thr) ? __float_as_uint(iou) + 1u : 0u;
                const unsigned m = wave_umax_dpp(key);
                int my_id;
                if (m != 0u) {
                    const int bj = __ffsll((long long)__ballot(key == m)) - 1;
                    my_id = __builtin_amdgcn_readlane(pidv, bj);
                    pidv = lane == bj ? -1 : pidv;      // claimed
                } else {
                    my_id = next_id++;
                }
                cid = lane == i ? my_id : cid;
            }
            outv = cid;                                 // lanes >= n keep -1
            pbx = cx; pby = cy; pbw = cw; pbh = ch; pbl = cl; pidv = cid; np = n;
        }
        for (int j = lane; j < cap; j += 64) id[(T - 1) * cap + j] = j < 64 ? outv : -1;
        if (lane == 0) nids[clip] = next_id;
        if constexpr (STREAM) store_slot(nullptr, outv);
        return;
    }
    // ---- general form (any count up to cap): previous / current frame in LDS ----
    if constexpr (STREAM) {
        for (int j = lane; j < np; j += 64) {
            const float *q = sb + j * 8;
            pb[j] = q[0]; pb[cap + j] = q[1]; pb[2 * cap + j] = q[2]; pb[3 * cap + j] = q[3]; pb[4 * cap + j] = q[5];
            pid[j] = si[j];
        }      // (the fence after frame 0's boxes below orders these too)
    }
    for (int t = 0; t < T; ++t) {
        const int n = min(cnt[t], cap);
        const float *cur = bx + (long long)t * cap * DT_BOX_FLOATS;
        for (int j = lane; j < n; j += 64) {
            const float *q = cur + j * 8;
            cb[j] = q[0]; cb[cap + j] = q[1]; cb[2 * cap + j] = q[2]; cb[3 * cap + j] = q[3]; cb[4 * cap + j] = q[5];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < n; ++i) {
            const float ax = cb[i], ay = cb[cap + i], aw = cb[2 * cap + i], ah = cb[3 * cap + i], al = cb[4 * cap + i];
            // best = largest IoU among the unclaimed same-label boxes of the previous frame, ties -> lowest j.  Per chunk
            // of 64 candidates: key = IoU bits + 1 (0 = not eligible; IoU >= 0, so the bit pattern orders like the value),
            // wave maximum by DPP row shifts + four lane reads, lowest lane holding it by ballot; a later chunk must be
            // strictly better to replace an earlier one.
            unsigned bestk = 0u;
            int bj = 0;
            for (int j0 = 0; j0 < np; j0 += 64) {
                const int j = j0 + lane;
                unsigned key = 0u;
                if (j < np && pid[j] >= 0 && pb[4 * cap + j] == al) {
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, pb[j], pb[cap + j], pb[2 * cap + j], pb[3 * cap + j]);
                    if (iou >= thr) key = __float_as_uint(iou) + 1u;
                }
                const unsigned m = wave_umax_dpp(key);
                if (m > bestk) {
                    bestk = m;
                    bj = j0 + __ffsll((long long)__ballot(key == m)) - 1;
                }
            }
            int my_id;
            if (bestk != 0u) {
                my_id = pid[bj];
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) pid[bj] = -1;            // claimed
            } else {
                my_id = next_id++;
            }
            if (lane == 0) cid[i] = my_id;
            __builtin_amdgcn_wave_barrier();
        }
        // publish this frame's ids, then it becomes the previous frame
        for (int j = lane; j < cap; j += 64) id[t * cap + j] = j < n ? cid[j] : -1;
        for (int j = lane; j < n; j += 64) {
            pb[j] = cb[j]; pb[cap + j] = cb[cap + j]; pb[2 * cap + j] = cb[2 * cap + j];
            pb[3 * cap + j] = cb[3 * cap + j]; pb[4 * cap + j] = cb[4 * cap + j];
            pid[j] = cid[j];
        }
        np = n;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) nids[clip] = next_id;
    if constexpr (STREAM) store_slot(pid, -1);
}

int launch_associate(hipStream_t st, const float *boxes, const int *counts, int n_clips, int T, int cap, float thr,
                     int *ids, int *nids)
{
    if (n_clips <= 0) return 0;
    const size_t lds = (size_t)cap * 12 * sizeof(float);   // 2 x 5 box fields + 2 id arrays
    if (lds > 160 * 1024) return 2;
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(associate_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024) != hipSuccess;
        }))
        return 1;
    hipLaunchKernelGGL(associate_kernel<false>, dim3((unsigned)n_clips), dim3(64), lds, st, boxes, counts, T, cap, thr, ids,
                       nids, AssocCarry{nullptr, nullptr, nullptr, nullptr, nullptr, 0});
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_associate_stream(hipStream_t st, const float *boxes, const int *counts, int n_clips, int T, int cap, float thr,
                            int *ids, int *nids, const AssocCarry &carry)
{
    if (n_clips <= 0) return 0;
    if (T <= 0 || !carry.slots) return 2;
    const size_t lds = (size_t)cap * 12 * sizeof(float);
    if (lds > 160 * 1024) return 2;
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(associate_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024) != hipSuccess;
        }))
        return 1;
    hipLaunchKernelGGL(associate_kernel<true>, dim3((unsigned)n_clips), dim3(64), lds, st, boxes, counts, T, cap, thr, ids,
                       nids, carry);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------
// Track identity with TRACK MEMORY (DESIGN.md "Track identity", max_age): a lost track keeps its id for up to max_age
// frames.  Per clip (or stream slot) a TRACK TABLE of at most tcap entries -- box, label, id, age = frames since the
// track last had a box -- takes the place of "the previous frame": box i takes the id of the unclaimed entry of the
// same label with age <= max_age and the largest IoU >= thr (ties -> lowest table index), else opens a new id;
// gap = the claimed entry's age (-1: new id).  After the frame the table is rebuilt: the frame's boxes in decode
// order (age 0), behind them the unclaimed entries with age + 1 <= max_age in their previous order; the cut at tcap
// drops the tail.  With max_age = 0 the table is the previous frame and this is associate_kernel's rule bit for bit.
// One wavefront per clip, two forms like associate_kernel.  A claimed entry is marked by id = -1 (ids are >= 0).
// ---------------------------------------------------------------------------
template <bool STREAM>
__global__ __launch_bounds__(64) void associate_mem_kernel(const float *boxes, const int *counts, int T, int cap, float thr,
                                                           int max_age, int tcap, int *ids, int *nids, int *gaps, AssocCarry carry)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int clip = blockIdx.x, lane = threadIdx.x;
    const float *bx = boxes + (long long)clip * T * cap * DT_BOX_FLOATS;
    const int *cnt = counts + (long long)clip * T;
    int *id = ids + (long long)clip * T * cap;
    int *gp = gaps ? gaps + (long long)clip * T * cap : nullptr;
    int next_id = 0;
    int nt = 0, n0 = 0;       // entries in the table; of them, leading entries of age 0 (the last frame's boxes)
    float *sb = nullptr;
    int *si = nullptr, *sa = nullptr, *sm = nullptr;
    if constexpr (STREAM) {
        const int slot = carry.slots[clip];
        sb = carry.boxes + (long long)slot * tcap * DT_BOX_FLOATS;
        si = carry.ids + (long long)slot * tcap;
        sa = carry.ages + (long long)slot * tcap;
        sm = carry.meta + slot * STREAM_META;
        const int w = sm[SM_COUNT];
        n0 = min(w & SM_COUNT_MASK, cap);
        nt = min(n0 + (int)((unsigned)w >> SM_AGED_SHIFT), tcap);
        next_id = sm[SM_NEXT_ID];
    }
    auto store_meta = [&]() {
        if (lane == 0) {
            sm[SM_COUNT] = n0 | ((nt - n0) << SM_AGED_SHIFT);
            sm[SM_NEXT_ID] = next_id;
            const int f = sm[SM_ASSOC_FRAMES];
            sm[SM_ASSOC_FRAMES] = f > (1 << 30) ? f : f + T;
        }
    };
    // ---- register form (tcap <= 64, hence every frame <= 64 boxes; T <= 64) ----
    // Lane j holds table entry j (box, label, id, age) and box j of the current frame.  The match is associate_kernel's chain with
    // `age <= max_age` in the eligibility test.  The rebuild is one ballot, one prefix count and seven ds_permute pushes: the kept
    // survivors go to lanes n .. n + kept - 1, every other lane to the lanes that are left, so the push is a permutation of the 64 lanes.
    if (tcap <= 64 && T <= 64) {
        const int cnt_l = lane < T ? min(cnt[lane], cap) : 0;
        auto request = [&](int t, float4 &q, float &ql) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float *src = bx + ((long long)t * cap + (lane < n ? lane : 0)) * DT_BOX_FLOATS;
            q = *reinterpret_cast<const float4 *>(src);
            ql = src[5];
        };
        float4 nq; float nl;
        request(0, nq, nl);
        float tbx = 0.0f, tby = 0.0f, tbw = 0.0f, tbh = 0.0f, tbl = 0.0f;
        int tid = -1, tage = 0, outv = -1, outg = -1;
        if constexpr (STREAM) {
            if (lane < nt) {
                const float *q = sb + lane * DT_BOX_FLOATS;
                const float4 v = *reinterpret_cast<const float4 *>(q);
                tbx = v.x; tby = v.y; tbw = v.z; tbh = v.w; tbl = q[5];
                tid = si[lane];
                tage = lane < n0 ? 0 : sa[lane];
            }
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int t = 0; t < T; ++t) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float cx = nq.x, cy = nq.y, cw = nq.z, ch = nq.w, cl = nl;        // waits for frame t's boxes
            if (t + 1 < T) request(t + 1, nq, nl);
            if (t > 0 && lane < cap) {
                id[(t - 1) * cap + lane] = outv;
                if (gp) gp[(t - 1) * cap + lane] = outg;
            }
            int cid = -1, cgap = -1;
            for (int i = 0; i < n; ++i) {
                const float ax = readlane_f(cx, i), ay = readlane_f(cy, i), aw = readlane_f(cw, i), ah = readlane_f(ch, i);
                const float al = readlane_f(cl, i);
                const float iou = bbox_iou_ref(ax, ay, aw, ah, tbx, tby, tbw, tbh);
                const unsigned key = (lane < nt && tid >= 0 && tage <= max_age && tbl == al && iou >= thr) ? __float_as_uint(iou) + 1u : 0u;
                const unsigned m = wave_umax_dpp(key);
                int my_id, my_gap = -1;
                if (m != 0u) {
                    const int bj = __ffsll((long long)__ballot(key == m)) - 1;
                    my_id = __builtin_amdgcn_readlane(tid, bj);
                    my_gap = __builtin_amdgcn_readlane(tage, bj);
                    tid = lane == bj ? -1 : tid;        // claimed
                } else {
                    my_id = next_id++;
                }
                cid = lane == i ? my_id : cid;
                cgap = lane == i ? my_gap : cgap;
            }
            outv = cid; outg = cgap;                    // lanes >= n keep -1
            // rebuild: frame t's boxes in lanes 0 .. n-1, the kept survivors behind them
            const bool surv = lane < nt && tid >= 0 && tage < max_age;
            const unsigned long long sm_ = __ballot(surv);
            const bool keep = surv && n + __popcll(sm_ & below) < tcap;
            const unsigned long long km = __ballot(keep);
            const int kept = __popcll(km);
            const int dst = keep ? n + __popcll(km & below) : n + kept + __popcll(~km & below);
            const int da = (dst & 63) << 2;
            const float px = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbx)));
            const float py = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tby)));
            const float pw = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbw)));
            const float ph = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbh)));
            const float pl = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbl)));
            const int pi = __builtin_amdgcn_ds_permute(da, tid);
            const int pa = __builtin_amdgcn_ds_permute(da, tage);
            const bool cur = lane < n;
            tbx = cur ? cx : px; tby = cur ? cy : py; tbw = cur ? cw : pw; tbh = cur ? ch : ph; tbl = cur ? cl : pl;
            tid = cur ? cid : pi;
            tage = cur ? 0 : pa + 1;
            nt = n + kept; n0 = n;      // lanes >= nt hold whatever the permutation left there: don't-care, every use above is guarded by `lane < nt`
        }
        if (lane < cap) {
            id[(T - 1) * cap + lane] = outv;
            if (gp) gp[(T - 1) * cap + lane] = outg;
        }
        if (lane == 0) nids[clip] = next_id;
        if constexpr (STREAM) {
            if (lane < nt) {
                float4 *q = reinterpret_cast<float4 *>(sb + lane * DT_BOX_FLOATS);
                q[0] = make_float4(tbx, tby, tbw, tbh);
                q[1] = make_float4(0.0f, tbl, 0.0f, 0.0f);
                si[lane] = tid;
                sa[lane] = tage;
            }
            store_meta();
        }
        return;
    }
    // ---- general form (any tcap): two tables in LDS, read and rebuilt in turn; the current frame's boxes are loaded straight into the
    // leading entries of the table under construction, where the rebuild wants them ----
    const int TS = 7 * tcap;                             // one table: [5][tcap] box fields | [tcap] ids | [tcap] ages
    float *A = smem, *B = smem + TS;
    volatile int *cgap = reinterpret_cast<volatile int *>(smem + 2 * TS);      // [cap] gaps of the current frame
    if constexpr (STREAM) {
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        for (int j = lane; j < nt; j += 64) {
            const float *q = sb + j * 8;
            A[j] = q[0]; A[tcap + j] = q[1]; A[2 * tcap + j] = q[2]; A[3 * tcap + j] = q[3]; A[4 * tcap + j] = q[5];
            aid[j] = si[j];
            aage[j] = j < n0 ? 0 : sa[j];
        }      // (the fence after frame 0's boxes below orders these too)
    }
    for (int t = 0; t < T; ++t) {
        const int n = min(cnt[t], cap);
        const float *cur = bx + (long long)t * cap * DT_BOX_FLOATS;
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        volatile int *bid = reinterpret_cast<volatile int *>(B + 5 * tcap), *bage = bid + tcap;
        for (int j = lane; j < n; j += 64) {
            const float *q = cur + j * 8;
            B[j] = q[0]; B[tcap + j] = q[1]; B[2 * tcap + j] = q[2]; B[3 * tcap + j] = q[3]; B[4 * tcap + j] = q[5];
            bage[j] = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < n; ++i) {
            const float ax = B[i], ay = B[tcap + i], aw = B[2 * tcap + i], ah = B[3 * tcap + i], al = B[4 * tcap + i];
            unsigned bestk = 0u;
            int bj = 0;
            for (int j0 = 0; j0 < nt; j0 += 64) {          // 64 candidates per pass, as associate_kernel
                const int j = j0 + lane;
                unsigned key = 0u;
                if (j < nt && aid[j] >= 0 && aage[j] <= max_age && A[4 * tcap + j] == al) {
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, A[j], A[tcap + j], A[2 * tcap + j], A[3 * tcap + j]);
                    if (iou >= thr) key = __float_as_uint(iou) + 1u;
                }
                const unsigned m = wave_umax_dpp(key);
                if (m > bestk) {
                    bestk = m;
                    bj = j0 + __ffsll((long long)__ballot(key == m)) - 1;
                }
            }
            int my_id, my_gap = -1;
            if (bestk != 0u) {
                my_id = aid[bj];
                my_gap = aage[bj];
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) aid[bj] = -1;            // claimed
            } else {
                my_id = next_id++;
            }
            if (lane == 0) { bid[i] = my_id; cgap[i] = my_gap; }
            __builtin_amdgcn_wave_barrier();
        }
        for (int j = lane; j < cap; j += 64) {
            id[t * cap + j] = j < n ? bid[j] : -1;
            if (gp) gp[t * cap + j] = j < n ? cgap[j] : -1;
        }
        // survivors, 64 entries per pass, compacted behind the frame's boxes by a wave scan
        int run = n;
        for (int j0 = 0; j0 < nt; j0 += 64) {
            const int j = j0 + lane;
            const bool surv = j < nt && aid[j] >= 0 && aage[j] < max_age;
            const unsigned long long bal = __ballot(surv);
            const int d = run + __popcll(bal & ((1ull << lane) - 1ull));
            if (surv && d < tcap) {
                B[d] = A[j]; B[tcap + d] = A[tcap + j]; B[2 * tcap + d] = A[2 * tcap + j]; B[3 * tcap + d] = A[3 * tcap + j];
                B[4 * tcap + d] = A[4 * tcap + j];
                bid[d] = aid[j];
                bage[d] = aage[j] + 1;
            }
            run += __popcll(bal);
        }
        nt = min(run, tcap); n0 = n;
        float *sw = A; A = B; B = sw;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) nids[clip] = next_id;
    if constexpr (STREAM) {
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        for (int j = lane; j < nt; j += 64) {
            float4 *q = reinterpret_cast<float4 *>(sb + j * DT_BOX_FLOATS);
            q[0] = make_float4(A[j], A[tcap + j], A[2 * tcap + j], A[3 * tcap + j]);
            q[1] = make_float4(0.0f, A[4 * tcap + j], 0.0f, 0.0f);
            si[j] = aid[j];
            sa[j] = aage[j];
        }
        store_meta();
    }
}

// dynamic LDS of associate_mem_kernel: none in the register form (tcap <= 64, T <= 64); general form: two tables of 7 words per entry and
// the frame's gaps.  More than 160 KB: launch_associate_mem refuses the arguments.
size_t assoc_mem_lds_bytes(int T, int cap, int tcap)
{
    return (tcap <= 64 && T <= 64) ? 0 : ((size_t)14 * tcap + cap) * sizeof(float);
}

// 0: launched; 1: device error; 2: argument error (nothing launched).  carry.slots == null: the stateless launch.
int launch_associate_mem(hipStream_t st, const float *boxes, const int *counts, int n_clips, int T, int cap, float thr,
                         int max_age, int tcap, int *ids, int *nids, int *gaps, const AssocCarry &carry)
{
    if (n_clips <= 0) return 0;
    if (T <= 0 || cap <= 0 || tcap < cap || tcap > SM_COUNT_MASK || max_age < 0) return 2;
    const bool stream = carry.slots != nullptr;
    if (stream && carry.tcap != tcap) return 2;
    const size_t lds = assoc_mem_lds_bytes(T, cap, tcap);
    if (lds > 160 * 1024) return 2;
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(associate_mem_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024) != hipSuccess ||
                   hipFuncSetAttribute(reinterpret_cast<const void *>(associate_mem_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024) != hipSuccess;
        }))
        return 1;
    if (stream)
        hipLaunchKernelGGL(associate_mem_kernel<true>, dim3((unsigned)n_clips), dim3(64), lds, st, boxes, counts, T, cap, thr, max_age,
                           tcap, ids, nids, gaps, carry);
    else
        hipLaunchKernelGGL(associate_mem_kernel<false>, dim3((unsigned)n_clips), dim3(64), lds, st, boxes, counts, T, cap, thr, max_age,
                           tcap, ids, nids, gaps, AssocCarry{nullptr, nullptr, nullptr, nullptr, nullptr, 0});
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------
// Track identity with TRACK MOTION (DESIGN.md "Track identity", motion gain): the track-memory rule above with every table
// entry matched where a constant velocity predicts it.  An entry carries, beside box, label, id and age, the velocity
// (vx, vy) of its box's x, y per frame.  With k = float(age + 1) the entry's PREDICTED box is (x + k*vx, y + k*vy, w, h)
// (one multiply, one add, each rounded: this file forms no FMA), and the match is associate_mem_kernel's with the IoU taken
// against the predicted box.  When box i claims entry j: o = (x_i - x_j) / k on the STORED x_j (the correctly rounded
// quotient), v_i = v_j + gain * (o - v_j); a box that opens a new id starts at rest.  The rebuild carries the velocities
// along.  gain = 0 leaves every velocity 0 and is associate_mem_kernel bit for bit.
// A sibling of associate_mem_kernel, same two forms, chosen by the launcher from tcap and T alone.
// STREAM: the slot's velocities live in carry.vel and are the table's only while carry.vstamp[slot] equals the slot's
// association frame counter, which every association entry advances and this kernel alone copies into the stamp -- so a
// table that dt_associate_stream / dt_associate_stream_mem has touched since reads as at rest.
// ---------------------------------------------------------------------------
template <bool STREAM>
__global__ __launch_bounds__(64) void associate_motion_kernel(const float *boxes, const int *counts, int T, int cap, float thr,
                                                              int max_age, int tcap, float gain, int *ids, int *nids, int *gaps,
                                                              AssocCarry carry)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int clip = blockIdx.x, lane = threadIdx.x;
    const float *bx = boxes + (long long)clip * T * cap * DT_BOX_FLOATS;
    const int *cnt = counts + (long long)clip * T;
    int *id = ids + (long long)clip * T * cap;
    int *gp = gaps ? gaps + (long long)clip * T * cap : nullptr;
    int next_id = 0;
    int nt = 0, n0 = 0;       // entries in the table; of them, leading entries of age 0 (the last frame's boxes)
    float *sb = nullptr, *sv = nullptr;
    int *si = nullptr, *sa = nullptr, *sm = nullptr, *ss = nullptr;
    bool vvalid = false;      // the slot's stored velocities belong to the table it holds
    if constexpr (STREAM) {
        const int slot = carry.slots[clip];
        sb = carry.boxes + (long long)slot * tcap * DT_BOX_FLOATS;
        si = carry.ids + (long long)slot * tcap;
        sa = carry.ages + (long long)slot * tcap;
        sv = carry.vel + (long long)slot * tcap * 2;
        sm = carry.meta + slot * STREAM_META;
        ss = carry.vstamp + slot;
        const int w = sm[SM_COUNT];
        n0 = min(w & SM_COUNT_MASK, cap);
        nt = min(n0 + (int)((unsigned)w >> SM_AGED_SHIFT), tcap);
        next_id = sm[SM_NEXT_ID];
        const int f = sm[SM_ASSOC_FRAMES];
        vvalid = f > 0 && f <= (1 << 30) && *ss == f;
    }
    auto store_meta = [&]() {
        if (lane == 0) {
            sm[SM_COUNT] = n0 | ((nt - n0) << SM_AGED_SHIFT);
            sm[SM_NEXT_ID] = next_id;
            const int f = sm[SM_ASSOC_FRAMES];
            const int f1 = f > (1 << 30) ? f : f + T;
            sm[SM_ASSOC_FRAMES] = f1;
            *ss = f1;                                   // (a saturated counter never validates: the test above)
        }
    };
    // ---- register form (tcap <= 64, hence every frame <= 64 boxes; T <= 64) ----
    // associate_mem_kernel's, with vx, vy in two more registers per lane.  The table does not change within a frame but for the
    // claims, so lane j predicts its entry once per frame, in front of the chain over the boxes.  On a claim the winner's stored
    // x, y, age, vx, vy reach every lane by v_readlane at the wave-uniform bj and lane i selects its new velocity; the rebuild
    // pushes nine values through ds_permute.
    if (tcap <= 64 && T <= 64) {
        const int cnt_l = lane < T ? min(cnt[lane], cap) : 0;
        auto request = [&](int t, float4 &q, float &ql) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float *src = bx + ((long long)t * cap + (lane < n ? lane : 0)) * DT_BOX_FLOATS;
            q = *reinterpret_cast<const float4 *>(src);
            ql = src[5];
        };
        float4 nq; float nl;
        request(0, nq, nl);
        float tbx = 0.0f, tby = 0.0f, tbw = 0.0f, tbh = 0.0f, tbl = 0.0f, tvx = 0.0f, tvy = 0.0f;
        int tid = -1, tage = 0, outv = -1, outg = -1;
        if constexpr (STREAM) {
            if (lane < nt) {
                const float *q = sb + lane * DT_BOX_FLOATS;
                const float4 v = *reinterpret_cast<const float4 *>(q);
                tbx = v.x; tby = v.y; tbw = v.z; tbh = v.w; tbl = q[5];
                tid = si[lane];
                tage = lane < n0 ? 0 : sa[lane];
                if (vvalid) {
                    const float2 w = *reinterpret_cast<const float2 *>(sv + lane * 2);
                    tvx = w.x; tvy = w.y;
                }
            }
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int t = 0; t < T; ++t) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float cx = nq.x, cy = nq.y, cw = nq.z, ch = nq.w, cl = nl;        // waits for frame t's boxes
            if (t + 1 < T) request(t + 1, nq, nl);
            if (t > 0 && lane < cap) {
                id[(t - 1) * cap + lane] = outv;
                if (gp) gp[(t - 1) * cap + lane] = outg;
            }
            // the entry's predicted place in this frame
            const float tk = (float)(tage + 1);
            const float qx = tbx + tk * tvx, qy = tby + tk * tvy;
            int cid = -1, cgap = -1;
            float cvx = 0.0f, cvy = 0.0f;
            for (int i = 0; i < n; ++i) {
                const float ax = readlane_f(cx, i), ay = readlane_f(cy, i), aw = readlane_f(cw, i), ah = readlane_f(ch, i);
                const float al = readlane_f(cl, i);
                const float iou = bbox_iou_ref(ax, ay, aw, ah, qx, qy, tbw, tbh);
                const unsigned key = (lane < nt && tid >= 0 && tage <= max_age && tbl == al && iou >= thr) ? __float_as_uint(iou) + 1u : 0u;
                const unsigned m = wave_umax_dpp(key);
                int my_id, my_gap = -1;
                float nvx = 0.0f, nvy = 0.0f;           // a new track starts at rest
                if (m != 0u) {
                    const int bj = __ffsll((long long)__ballot(key == m)) - 1;
                    my_id = __builtin_amdgcn_readlane(tid, bj);
                    my_gap = __builtin_amdgcn_readlane(tage, bj);
                    const float ex = readlane_f(tbx, bj), ey = readlane_f(tby, bj);
                    const float evx = readlane_f(tvx, bj), evy = readlane_f(tvy, bj);
                    const float k = (float)(my_gap + 1);
                    const float ox = (ax - ex) / k, oy = (ay - ey) / k;
                    nvx = evx + gain * (ox - evx);
                    nvy = evy + gain * (oy - evy);
                    tid = lane == bj ? -1 : tid;        // claimed
                } else {
                    my_id = next_id++;
                }
                cid = lane == i ? my_id : cid;
                cgap = lane == i ? my_gap : cgap;
                cvx = lane == i ? nvx : cvx;
                cvy = lane == i ? nvy : cvy;
            }
            outv = cid; outg = cgap;                    // lanes >= n keep -1
            // rebuild: frame t's boxes in lanes 0 .. n-1, the kept survivors behind them (associate_mem_kernel's permutation)
            const bool surv = lane < nt && tid >= 0 && tage < max_age;
            const unsigned long long sm_ = __ballot(surv);
            const bool keep = surv && n + __popcll(sm_ & below) < tcap;
            const unsigned long long km = __ballot(keep);
            const int kept = __popcll(km);
            const int dst = keep ? n + __popcll(km & below) : n + kept + __popcll(~km & below);
            const int da = (dst & 63) << 2;
            const float px = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbx)));
            const float py = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tby)));
            const float pw = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbw)));
            const float ph = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbh)));
            const float pl = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbl)));
            const float pvx = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tvx)));
            const float pvy = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tvy)));
            const int pi = __builtin_amdgcn_ds_permute(da, tid);
            const int pa = __builtin_amdgcn_ds_permute(da, tage);
            const bool cur = lane < n;
            tbx = cur ? cx : px; tby = cur ? cy : py; tbw = cur ? cw : pw; tbh = cur ? ch : ph; tbl = cur ? cl : pl;
            tvx = cur ? cvx : pvx; tvy = cur ? cvy : pvy;
            tid = cur ? cid : pi;
            tage = cur ? 0 : pa + 1;
            nt = n + kept; n0 = n;      // lanes >= nt: don't-care, every use above is guarded by `lane < nt`
        }
        if (lane < cap) {
            id[(T - 1) * cap + lane] = outv;
            if (gp) gp[(T - 1) * cap + lane] = outg;
        }
        if (lane == 0) nids[clip] = next_id;
        if constexpr (STREAM) {
            if (lane < nt) {
                float4 *q = reinterpret_cast<float4 *>(sb + lane * DT_BOX_FLOATS);
                q[0] = make_float4(tbx, tby, tbw, tbh);
                q[1] = make_float4(0.0f, tbl, 0.0f, 0.0f);
                si[lane] = tid;
                sa[lane] = tage;
                *reinterpret_cast<float2 *>(sv + lane * 2) = make_float2(tvx, tvy);
            }
            store_meta();
        }
        return;
    }
    // ---- general form (any tcap): associate_mem_kernel's two LDS tables, of nine words per entry ----
    const int TS = 9 * tcap;                             // one table: [5][tcap] box fields | [tcap] ids | [tcap] ages | [2][tcap] vx, vy
    float *A = smem, *B = smem + TS;
    volatile int *cgap = reinterpret_cast<volatile int *>(smem + 2 * TS);      // [cap] gaps of the current frame
    if constexpr (STREAM) {
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        for (int j = lane; j < nt; j += 64) {
            const float *q = sb + j * 8;
            A[j] = q[0]; A[tcap + j] = q[1]; A[2 * tcap + j] = q[2]; A[3 * tcap + j] = q[3]; A[4 * tcap + j] = q[5];
            aid[j] = si[j];
            aage[j] = j < n0 ? 0 : sa[j];
            A[7 * tcap + j] = vvalid ? sv[2 * j] : 0.0f;
            A[8 * tcap + j] = vvalid ? sv[2 * j + 1] : 0.0f;
        }      // (the fence after frame 0's boxes below orders these too)
    }
    for (int t = 0; t < T; ++t) {
        const int n = min(cnt[t], cap);
        const float *cur = bx + (long long)t * cap * DT_BOX_FLOATS;
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        volatile int *bid = reinterpret_cast<volatile int *>(B + 5 * tcap), *bage = bid + tcap;
        for (int j = lane; j < n; j += 64) {
            const float *q = cur + j * 8;
            B[j] = q[0]; B[tcap + j] = q[1]; B[2 * tcap + j] = q[2]; B[3 * tcap + j] = q[3]; B[4 * tcap + j] = q[5];
            bage[j] = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < n; ++i) {
            const float ax = B[i], ay = B[tcap + i], aw = B[2 * tcap + i], ah = B[3 * tcap + i], al = B[4 * tcap + i];
            unsigned bestk = 0u;
            int bj = 0;
            for (int j0 = 0; j0 < nt; j0 += 64) {          // 64 candidates per pass, as associate_kernel
                const int j = j0 + lane;
                unsigned key = 0u;
                if (j < nt && aid[j] >= 0 && aage[j] <= max_age && A[4 * tcap + j] == al) {
                    const float k = (float)(aage[j] + 1);
                    const float qx = A[j] + k * A[7 * tcap + j], qy = A[tcap + j] + k * A[8 * tcap + j];
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, qx, qy, A[2 * tcap + j], A[3 * tcap + j]);
                    if (iou >= thr) key = __float_as_uint(iou) + 1u;
                }
                const unsigned m = wave_umax_dpp(key);
                if (m > bestk) {
                    bestk = m;
                    bj = j0 + __ffsll((long long)__ballot(key == m)) - 1;
                }
            }
            int my_id, my_gap = -1;
            float nvx = 0.0f, nvy = 0.0f;               // a new track starts at rest
            if (bestk != 0u) {
                my_id = aid[bj];
                my_gap = aage[bj];
                const float evx = A[7 * tcap + bj], evy = A[8 * tcap + bj];
                const float k = (float)(my_gap + 1);
                const float ox = (ax - A[bj]) / k, oy = (ay - A[tcap + bj]) / k;
                nvx = evx + gain * (ox - evx);
                nvy = evy + gain * (oy - evy);
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) aid[bj] = -1;            // claimed
            } else {
                my_id = next_id++;
            }
            if (lane == 0) { bid[i] = my_id; cgap[i] = my_gap; B[7 * tcap + i] = nvx; B[8 * tcap + i] = nvy; }
            __builtin_amdgcn_wave_barrier();
        }
        for (int j = lane; j < cap; j += 64) {
            id[t * cap + j] = j < n ? bid[j] : -1;
            if (gp) gp[t * cap + j] = j < n ? cgap[j] : -1;
        }
        // survivors, 64 entries per pass, compacted behind the frame's boxes by a wave scan
        int run = n;
        for (int j0 = 0; j0 < nt; j0 += 64) {
            const int j = j0 + lane;
            const bool surv = j < nt && aid[j] >= 0 && aage[j] < max_age;
            const unsigned long long bal = __ballot(surv);
            const int d = run + __popcll(bal & ((1ull << lane) - 1ull));
            if (surv && d < tcap) {
                B[d] = A[j]; B[tcap + d] = A[tcap + j]; B[2 * tcap + d] = A[2 * tcap + j]; B[3 * tcap + d] = A[3 * tcap + j];
                B[4 * tcap + d] = A[4 * tcap + j];
                bid[d] = aid[j];
                bage[d] = aage[j] + 1;
                B[7 * tcap + d] = A[7 * tcap + j]; B[8 * tcap + d] = A[8 * tcap + j];
            }
            run += __popcll(bal);
        }
        nt = min(run, tcap); n0 = n;
        float *sw = A; A = B; B = sw;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) nids[clip] = next_id;
    if constexpr (STREAM) {
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        for (int j = lane; j < nt; j += 64) {
            float4 *q = reinterpret_cast<float4 *>(sb + j * DT_BOX_FLOATS);
            q[0] = make_float4(A[j], A[tcap + j], A[2 * tcap + j], A[3 * tcap + j]);
            q[1] = make_float4(0.0f, A[4 * tcap + j], 0.0f, 0.0f);
            si[j] = aid[j];
            sa[j] = aage[j];
            *reinterpret_cast<float2 *>(sv + j * 2) = make_float2(A[7 * tcap + j], A[8 * tcap + j]);
        }
        store_meta();
    }
}

// dynamic LDS of associate_motion_kernel: none in the register form (tcap <= 64, T <= 64); general form: two tables of 9 words per entry
// and the frame's gaps.  More than 160 KB: launch_associate_motion refuses the arguments.
size_t assoc_motion_lds_bytes(int T, int cap, int tcap)
{
    return (tcap <= 64 && T <= 64) ? 0 : ((size_t)18 * tcap + cap) * sizeof(float);
}

// 0: launched; 1: device error; 2: argument error (nothing launched).  carry.slots == null: the stateless launch.
int launch_associate_motion(hipStream_t st, const float *boxes, const int *counts, int n_clips, int T, int cap, float thr,
                            int max_age, int tcap, float gain, int *ids, int *nids, int *gaps, const AssocCarry &carry)
{
    if (n_clips <= 0) return 0;
    if (T <= 0 || cap <= 0 || tcap < cap || tcap > SM_COUNT_MASK || max_age < 0) return 2;
    if (!(gain >= 0.0f && gain <= 1.0f)) return 2;      // (NaN fails both comparisons)
    const bool stream = carry.slots != nullptr;
    if (stream && (carry.tcap != tcap || !carry.vel || !carry.vstamp)) return 2;
    const size_t lds = assoc_motion_lds_bytes(T, cap, tcap);
    if (lds > 160 * 1024) return 2;
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(associate_motion_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024) != hipSuccess ||
                   hipFuncSetAttribute(reinterpret_cast<const void *>(associate_motion_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024) != hipSuccess;
        }))
        return 1;
    if (stream)
        hipLaunchKernelGGL(associate_motion_kernel<true>, dim3((unsigned)n_clips), dim3(64), lds, st, boxes, counts, T, cap, thr, max_age,
                           tcap, gain, ids, nids, gaps, carry);
    else
        hipLaunchKernelGGL(associate_motion_kernel<false>, dim3((unsigned)n_clips), dim3(64), lds, st, boxes, counts, T, cap, thr, max_age,
                           tcap, gain, ids, nids, gaps, AssocCarry{nullptr, nullptr, nullptr, nullptr, nullptr, 0});
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------
// Track identity with a TRACK READ-OUT (DESIGN.md "Track identity", track read-out): the track-motion rule above, bit for bit, with
// one more word per table entry -- HITS, the frames in which the track had a box -- and the table written out once per frame.
// A box that opens a new id starts at hits = 1, a box that claims entry j carries hits_j + 1, an unclaimed survivor keeps its
// hits; hits take no part in the match.  After frame t's rebuild (the cut at tcap included) the table is walked in table order
// and every CONFIRMED entry (hits >= min_hits) becomes one row of out.tracks / out.tinfo, compacted: x, y, w, h, label, vx, vy, 0
// and id, age, hits, box.  An entry of age 0 reports its stored x, y; one of age a >= 1 reports x + float(a)*vx, y + float(a)*vy
// (one multiply, one add, each rounded).  Rows from the count on are written zero / -1: every row of the frame is written once.
// A sibling of associate_motion_kernel, same two forms, chosen by the launcher from tcap and T alone.
// STREAM: the slot's hits live in carry.hits and are the table's only while carry.hstamp[slot] equals the slot's association
// frame counter; this kernel writes both stamps, associate_motion_kernel the velocity stamp alone -- after it every entry reads
// as hits = 1.
// MATCH (DESIGN.md "Track identity", track match policy): DT_MATCH_* bits chosen by the call, a template parameter so that 0 is the
// code this kernel had.  ANY_LABEL drops the label comparison from the candidate test.  BEST_FIRST replaces the match block of each
// form: instead of the boxes in decode order, the candidate pair (box, entry) with the largest IoU key is taken repeatedly, ties to
// the lowest box, then the lowest entry; the boxes left over open their ids in decode order afterwards.  Load, rebuild, hits,
// read-out and store are shared by all four.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void track_row_store(float *tracks, int *tinfo, long long row, float x, float y, float w, float h, float l,
                                                float vx, float vy, int id, int age, int hits, int box)
{
    float4 *q = reinterpret_cast<float4 *>(tracks + row * DT_TRACK_FLOATS);
    q[0] = make_float4(x, y, w, h);
    q[1] = make_float4(l, vx, vy, 0.0f);
    *reinterpret_cast<int4 *>(tinfo + row * DT_TRACK_INTS) = make_int4(id, age, hits, box);
}
__device__ __forceinline__ void track_row_empty(float *tracks, int *tinfo, long long row)
{
    track_row_store(tracks, tinfo, row, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1, -1, -1, -1);
}

template <bool STREAM, int MATCH>
__global__ __launch_bounds__(64) void associate_tracks_kernel(const float *boxes, const int *counts, int T, int cap, float thr,
                                                              int max_age, int tcap, float gain, int min_hits, int *ids, int *nids,
                                                              int *gaps, TrackReadout out, AssocCarry carry)
{
    constexpr bool BEST = (MATCH & DT_MATCH_BEST_FIRST) != 0, ANY = (MATCH & DT_MATCH_ANY_LABEL) != 0;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int clip = blockIdx.x, lane = threadIdx.x;
    const float *bx = boxes + (long long)clip * T * cap * DT_BOX_FLOATS;
    const int *cnt = counts + (long long)clip * T;
    int *id = ids + (long long)clip * T * cap;
    int *gp = gaps ? gaps + (long long)clip * T * cap : nullptr;
    int *hp = out.hits ? out.hits + (long long)clip * T * cap : nullptr;
    // the read-out of this clip: rows [T][tcap]; null = no read-out
    float *tk = out.tracks ? out.tracks + (long long)clip * T * tcap * DT_TRACK_FLOATS : nullptr;
    int *ti = out.tracks ? out.tinfo + (long long)clip * T * tcap * DT_TRACK_INTS : nullptr;
    int *tc = out.tracks ? out.tcounts + (long long)clip * T : nullptr;
    int next_id = 0;
    int nt = 0, n0 = 0;       // entries in the table; of them, leading entries of age 0 (the last frame's boxes)
    float *sb = nullptr, *sv = nullptr;
    int *si = nullptr, *sa = nullptr, *sm = nullptr, *ss = nullptr, *sh = nullptr, *shs = nullptr;
    bool vvalid = false;      // the slot's stored velocities belong to the table it holds
    bool hvalid = false;      // ... and so do its stored hits
    if constexpr (STREAM) {
        const int slot = carry.slots[clip];
        sb = carry.boxes + (long long)slot * tcap * DT_BOX_FLOATS;
        si = carry.ids + (long long)slot * tcap;
        sa = carry.ages + (long long)slot * tcap;
        sv = carry.vel + (long long)slot * tcap * 2;
        sh = carry.hits + (long long)slot * tcap;
        sm = carry.meta + slot * STREAM_META;
        ss = carry.vstamp + slot;
        shs = carry.hstamp + slot;
        const int w = sm[SM_COUNT];
        n0 = min(w & SM_COUNT_MASK, cap);
        nt = min(n0 + (int)((unsigned)w >> SM_AGED_SHIFT), tcap);
        next_id = sm[SM_NEXT_ID];
        const int f = sm[SM_ASSOC_FRAMES];
        const bool fok = f > 0 && f <= (1 << 30);
        vvalid = fok && *ss == f;
        hvalid = fok && *shs == f;
    }
    auto store_meta = [&]() {
        if (lane == 0) {
            sm[SM_COUNT] = n0 | ((nt - n0) << SM_AGED_SHIFT);
            sm[SM_NEXT_ID] = next_id;
            const int f = sm[SM_ASSOC_FRAMES];
            const int f1 = f > (1 << 30) ? f : f + T;
            sm[SM_ASSOC_FRAMES] = f1;
            *ss = f1;                                   // (a saturated counter never validates: the test above)
            *shs = f1;
        }
    };
    // ---- register form (tcap <= 64, hence every frame <= 64 boxes; T <= 64) ----
    // associate_motion_kernel's, with hits in one more register per lane and one more ds_permute in the rebuild.  The read-out
    // follows the rebuild: a ballot of the confirmed lanes, a popcount below the lane, and every lane writes one row -- a
    // confirmed lane its own, the others the empty rows behind the count.  Frame t + 1's boxes were requested at the top of
    // iteration t, in front of these stores, so the wait for them at the top of t + 1 does not wait for the read-out.
    if (tcap <= 64 && T <= 64) {
        const int cnt_l = lane < T ? min(cnt[lane], cap) : 0;
        auto request = [&](int t, float4 &q, float &ql) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float *src = bx + ((long long)t * cap + (lane < n ? lane : 0)) * DT_BOX_FLOATS;
            q = *reinterpret_cast<const float4 *>(src);
            ql = src[5];
        };
        float4 nq; float nl;
        request(0, nq, nl);
        float tbx = 0.0f, tby = 0.0f, tbw = 0.0f, tbh = 0.0f, tbl = 0.0f, tvx = 0.0f, tvy = 0.0f;
        int tid = -1, tage = 0, thits = 0, outv = -1, outg = -1, outh = -1;
        if constexpr (STREAM) {
            if (lane < nt) {
                const float *q = sb + lane * DT_BOX_FLOATS;
                const float4 v = *reinterpret_cast<const float4 *>(q);
                tbx = v.x; tby = v.y; tbw = v.z; tbh = v.w; tbl = q[5];
                tid = si[lane];
                tage = lane < n0 ? 0 : sa[lane];
                if (vvalid) {
                    const float2 w = *reinterpret_cast<const float2 *>(sv + lane * 2);
                    tvx = w.x; tvy = w.y;
                }
                thits = hvalid ? sh[lane] : 1;
            }
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int t = 0; t < T; ++t) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float cx = nq.x, cy = nq.y, cw = nq.z, ch = nq.w, cl = nl;        // waits for frame t's boxes
            if (t + 1 < T) request(t + 1, nq, nl);
            if (t > 0 && lane < cap) {
                id[(t - 1) * cap + lane] = outv;
                if (gp) gp[(t - 1) * cap + lane] = outg;
                if (hp) hp[(t - 1) * cap + lane] = outh;
            }
            // the entry's predicted place in this frame
            const float tk_ = (float)(tage + 1);
            const float qx = tbx + tk_ * tvx, qy = tby + tk_ * tvy;
            int cid = -1, cgap = -1, chits = -1;
            float cvx = 0.0f, cvy = 0.0f;
            if constexpr (BEST) {
                // best-IoU-first order: the frame's keys are an [n][64] tile of dynamic LDS, column = lane = entry, and a lane
                // reads and writes its own column only.  Each lane caches its column's best remaining (key, box), ties to the
                // lowest box.  A round: the wave-wide largest cached key, among its lanes the lowest box, among those the
                // lowest lane; box bi claims entry bj; the lanes whose cached box was bi walk their column again.  The rounds only
                // note the claim (lane bi keeps bj): what the box inherits is fetched and computed once per frame behind them,
                // lane = box, with the decode-order loop's operations on the same operands.
                unsigned *km = reinterpret_cast<unsigned *>(smem) + lane;
                const bool live = lane < nt && tid >= 0 && tage <= max_age;
                unsigned bk = 0u;
                int bb = 0;
                for (int i = 0; i < n; ++i) {
                    const float ax = readlane_f(cx, i), ay = readlane_f(cy, i), aw = readlane_f(cw, i), ah = readlane_f(ch, i);
                    const float al = readlane_f(cl, i);
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, qx, qy, tbw, tbh);
                    const unsigned key = (live && (ANY || tbl == al) && iou >= thr) ? __float_as_uint(iou) + 1u : 0u;
                    km[i * 64] = key;
                    if (key > bk) { bk = key; bb = i; }
                }
                unsigned long long taken = 0ull;        // boxes that have claimed an entry
                const int tid0 = tid;                   // the entries' ids before the claims mark them
                int cent = -1;                          // lane = box: the entry it claimed
                for (;;) {
                    const unsigned m = wave_umax_dpp(bk);
                    if (m == 0u) break;
                    const int bi = 64 - (int)wave_umax_dpp(bk == m ? (unsigned)(64 - bb) : 0u);
                    const int bj = __ffsll((long long)__ballot(bk == m && bb == bi)) - 1;
                    cent = lane == bi ? bj : cent;
                    taken |= 1ull << bi;
                    if (lane == bj) {
                        tid = -1;                       // claimed
                        bk = 0u;
                    } else if (bk != 0u && bb == bi) {
                        bk = 0u;
                        for (int i = 0; i < n; i += 4) {        // four keys of the column in flight
                            unsigned k4[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) k4[u] = km[min(i + u, n - 1) * 64];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int iu = i + u;
                                const unsigned key = (iu < n && !((taken >> (iu & 63)) & 1ull)) ? k4[u] : 0u;
                                if (key > bk) { bk = key; bb = iu; }
                            }
                        }
                    }
                }
                // what a box inherits from the entry it claimed (every lane takes part in the lane reads)
                {
                    const int src = (cent >= 0 ? cent : 0) << 2;
                    const int e_id = __builtin_amdgcn_ds_bpermute(src, tid0);
                    const int e_age = __builtin_amdgcn_ds_bpermute(src, tage);
                    const int e_hits = __builtin_amdgcn_ds_bpermute(src, thits);
                    const float ex = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(tbx)));
                    const float ey = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(tby)));
                    const float evx = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(tvx)));
                    const float evy = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(tvy)));
                    if (cent >= 0) {
                        const float k = (float)(e_age + 1);
                        const float ox = (cx - ex) / k, oy = (cy - ey) / k;
                        cid = e_id; cgap = e_age; chits = e_hits + 1;
                        cvx = evx + gain * (ox - evx);
                        cvy = evy + gain * (oy - evy);
                    }
                }
                // the boxes that claimed nothing open ids in decode order, at hits = 1 and at rest
                const bool fresh = lane < n && cent < 0;
                const unsigned long long fm = __ballot(fresh);
                if (fresh) { cid = next_id + __popcll(fm & below); cgap = -1; chits = 1; }
                next_id += __popcll(fm);
            } else
            for (int i = 0; i < n; ++i) {
                const float ax = readlane_f(cx, i), ay = readlane_f(cy, i), aw = readlane_f(cw, i), ah = readlane_f(ch, i);
                const float al = readlane_f(cl, i);
                const float iou = bbox_iou_ref(ax, ay, aw, ah, qx, qy, tbw, tbh);
                const unsigned key = (lane < nt && tid >= 0 && tage <= max_age && (ANY || tbl == al) && iou >= thr) ? __float_as_uint(iou) + 1u : 0u;
                const unsigned m = wave_umax_dpp(key);
                int my_id, my_gap = -1, my_hits = 1;    // a new track: one frame with a box
                float nvx = 0.0f, nvy = 0.0f;           // ... and at rest
                if (m != 0u) {
                    const int bj = __ffsll((long long)__ballot(key == m)) - 1;
                    my_id = __builtin_amdgcn_readlane(tid, bj);
                    my_gap = __builtin_amdgcn_readlane(tage, bj);
                    my_hits = __builtin_amdgcn_readlane(thits, bj) + 1;
                    const float ex = readlane_f(tbx, bj), ey = readlane_f(tby, bj);
                    const float evx = readlane_f(tvx, bj), evy = readlane_f(tvy, bj);
                    const float k = (float)(my_gap + 1);
                    const float ox = (ax - ex) / k, oy = (ay - ey) / k;
                    nvx = evx + gain * (ox - evx);
                    nvy = evy + gain * (oy - evy);
                    tid = lane == bj ? -1 : tid;        // claimed
                } else {
                    my_id = next_id++;
                }
                cid = lane == i ? my_id : cid;
                cgap = lane == i ? my_gap : cgap;
                chits = lane == i ? my_hits : chits;
                cvx = lane == i ? nvx : cvx;
                cvy = lane == i ? nvy : cvy;
            }
            outv = cid; outg = cgap; outh = chits;      // lanes >= n keep -1
            // rebuild: frame t's boxes in lanes 0 .. n-1, the kept survivors behind them (associate_mem_kernel's permutation)
            const bool surv = lane < nt && tid >= 0 && tage < max_age;
            const unsigned long long sm_ = __ballot(surv);
            const bool keep = surv && n + __popcll(sm_ & below) < tcap;
            const unsigned long long km = __ballot(keep);
            const int kept = __popcll(km);
            const int dst = keep ? n + __popcll(km & below) : n + kept + __popcll(~km & below);
            const int da = (dst & 63) << 2;
            const float px = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbx)));
            const float py = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tby)));
            const float pw = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbw)));
            const float ph = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbh)));
            const float pl = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tbl)));
            const float pvx = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tvx)));
            const float pvy = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tvy)));
            const int pi = __builtin_amdgcn_ds_permute(da, tid);
            const int pa = __builtin_amdgcn_ds_permute(da, tage);
            const int phit = __builtin_amdgcn_ds_permute(da, thits);
            const bool cur = lane < n;
            tbx = cur ? cx : px; tby = cur ? cy : py; tbw = cur ? cw : pw; tbh = cur ? ch : ph; tbl = cur ? cl : pl;
            tvx = cur ? cvx : pvx; tvy = cur ? cvy : pvy;
            tid = cur ? cid : pi;
            tage = cur ? 0 : pa + 1;
            thits = cur ? chits : phit;
            nt = n + kept; n0 = n;      // lanes >= nt: don't-care, every use above and below is guarded by `lane < nt`
            // read-out of the table as it now stands; lane = table index, so an age-0 entry's box index is the lane
            if (tk) {
                const bool conf = lane < nt && thits >= min_hits;
                const unsigned long long cm = __ballot(conf);
                const int nc = __popcll(cm);
                const int row = conf ? __popcll(cm & below) : nc + __popcll(~cm & below);
                if (row < tcap) {
                    const long long r = (long long)t * tcap + row;
                    if (conf) {
                        const float fa = (float)tage;
                        const float rx = cur ? tbx : tbx + fa * tvx, ry = cur ? tby : tby + fa * tvy;
                        track_row_store(tk, ti, r, rx, ry, tbw, tbh, tbl, tvx, tvy, tid, tage, thits, cur ? lane : -1);
                    } else {
                        track_row_empty(tk, ti, r);
                    }
                }
                if (lane == 0) tc[t] = nc;
            }
        }
        if (lane < cap) {
            id[(T - 1) * cap + lane] = outv;
            if (gp) gp[(T - 1) * cap + lane] = outg;
            if (hp) hp[(T - 1) * cap + lane] = outh;
        }
        if (lane == 0) nids[clip] = next_id;
        if constexpr (STREAM) {
            if (lane < nt) {
                float4 *q = reinterpret_cast<float4 *>(sb + lane * DT_BOX_FLOATS);
                q[0] = make_float4(tbx, tby, tbw, tbh);
                q[1] = make_float4(0.0f, tbl, 0.0f, 0.0f);
                si[lane] = tid;
                sa[lane] = tage;
                *reinterpret_cast<float2 *>(sv + lane * 2) = make_float2(tvx, tvy);
                sh[lane] = thits;
            }
            store_meta();
        }
        return;
    }
    // ---- general form (any tcap): associate_motion_kernel's two LDS tables, of ten words per entry ----
    const int TS = 10 * tcap;                            // one table: [5][tcap] box fields | [tcap] ids | [tcap] ages | [2][tcap] vx, vy | [tcap] hits
    float *A = smem, *B = smem + TS;
    volatile int *cgap = reinterpret_cast<volatile int *>(smem + 2 * TS);      // [cap] gaps of the current frame
    // best-IoU-first order only: per box its best remaining candidate (key, entry) and whether it has claimed one, [cap] each
    volatile unsigned *bkey = reinterpret_cast<volatile unsigned *>(smem + 2 * TS + cap);
    volatile int *bent = reinterpret_cast<volatile int *>(smem + 2 * TS + 2 * cap);
    volatile int *bdone = reinterpret_cast<volatile int *>(smem + 2 * TS + 3 * cap);
    // read-out of table A (nt entries, as frame t left it): 64 entries per pass compacted by a running count, the way the survivor
    // pass compacts; then the empty rows behind the count.  Called once the NEXT frame's boxes have been fetched (below), so these
    // stores stand behind those loads and never in front of them.
    auto readout = [&](int t) {
        volatile const int *aid = reinterpret_cast<volatile const int *>(A + 5 * tcap), *aage = aid + tcap;
        volatile const int *ahit = reinterpret_cast<volatile const int *>(A + 9 * tcap);
        int run = 0;
        for (int j0 = 0; j0 < nt; j0 += 64) {
            const int j = j0 + lane;
            const bool conf = j < nt && ahit[j] >= min_hits;
            const unsigned long long bal = __ballot(conf);
            if (conf) {
                const long long r = (long long)t * tcap + run + __popcll(bal & ((1ull << lane) - 1ull));
                const int age = aage[j];
                const float fa = (float)age;
                const float x = A[j], y = A[tcap + j], vx = A[7 * tcap + j], vy = A[8 * tcap + j];
                const float rx = age == 0 ? x : x + fa * vx, ry = age == 0 ? y : y + fa * vy;
                track_row_store(tk, ti, r, rx, ry, A[2 * tcap + j], A[3 * tcap + j], A[4 * tcap + j], vx, vy, aid[j], age, ahit[j],
                                age == 0 ? j : -1);
            }
            run += __popcll(bal);
        }
        for (int j = run + lane; j < tcap; j += 64) track_row_empty(tk, ti, (long long)t * tcap + j);
        if (lane == 0) tc[t] = run;
    };
    if constexpr (STREAM) {
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        volatile int *ahit = reinterpret_cast<volatile int *>(A + 9 * tcap);
        for (int j = lane; j < nt; j += 64) {
            const float *q = sb + j * 8;
            A[j] = q[0]; A[tcap + j] = q[1]; A[2 * tcap + j] = q[2]; A[3 * tcap + j] = q[3]; A[4 * tcap + j] = q[5];
            aid[j] = si[j];
            aage[j] = j < n0 ? 0 : sa[j];
            A[7 * tcap + j] = vvalid ? sv[2 * j] : 0.0f;
            A[8 * tcap + j] = vvalid ? sv[2 * j + 1] : 0.0f;
            ahit[j] = hvalid ? sh[j] : 1;
        }      // (the fence after frame 0's boxes below orders these too)
    }
    for (int t = 0; t < T; ++t) {
        const int n = min(cnt[t], cap);
        const float *cur = bx + (long long)t * cap * DT_BOX_FLOATS;
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        volatile int *ahit = reinterpret_cast<volatile int *>(A + 9 * tcap);
        volatile int *bid = reinterpret_cast<volatile int *>(B + 5 * tcap), *bage = bid + tcap;
        volatile int *bhit = reinterpret_cast<volatile int *>(B + 9 * tcap);
        for (int j = lane; j < n; j += 64) {
            const float *q = cur + j * 8;
            B[j] = q[0]; B[tcap + j] = q[1]; B[2 * tcap + j] = q[2]; B[3 * tcap + j] = q[3]; B[4 * tcap + j] = q[5];
            bage[j] = 0;
            if constexpr (BEST) bdone[j] = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (tk && t > 0) readout(t - 1);                  // table A is frame t-1's until the first claim below
        if constexpr (BEST) {
            // best-IoU-first order.  scan(i): box i's best candidate among the unclaimed entries, 64 entries per pass, ties to the
            // lowest entry -- the decode-order match's inner loop -- cached in bkey / bent.  A round: the largest cached key over
            // the boxes, 64 per pass, ties to the lowest box; that box claims its cached entry; the boxes still unmatched whose
            // cached entry it was are scanned again.  A matched box's key is 0, so the rounds end when no candidate is left.
            // A claim marks the entry by complementing its id (negative, like the decode-order loop's -1, and still readable)
            // and leaves the box's cached entry standing; what the boxes inherit is computed behind the rounds, lane = box.
            auto scan = [&](int i) {
                const float ax = B[i], ay = B[tcap + i], aw = B[2 * tcap + i], ah = B[3 * tcap + i], al = B[4 * tcap + i];
                unsigned bestk = 0u;
                int bj = 0;
                for (int j0 = 0; j0 < nt; j0 += 64) {
                    const int j = j0 + lane;
                    unsigned key = 0u;
                    if (j < nt && aid[j] >= 0 && aage[j] <= max_age && (ANY || A[4 * tcap + j] == al)) {
                        const float k = (float)(aage[j] + 1);
                        const float qx = A[j] + k * A[7 * tcap + j], qy = A[tcap + j] + k * A[8 * tcap + j];
                        const float iou = bbox_iou_ref(ax, ay, aw, ah, qx, qy, A[2 * tcap + j], A[3 * tcap + j]);
                        if (iou >= thr) key = __float_as_uint(iou) + 1u;
                    }
                    const unsigned m = wave_umax_dpp(key);
                    if (m > bestk) {
                        bestk = m;
                        bj = j0 + __ffsll((long long)__ballot(key == m)) - 1;
                    }
                }
                if (lane == 0) { bkey[i] = bestk; bent[i] = bj; }
            };
            for (int i = 0; i < n; ++i) scan(i);
            __builtin_amdgcn_wave_barrier();
            for (;;) {
                unsigned bestk = 0u;
                int bi = 0;
                for (int i0 = 0; i0 < n; i0 += 64) {
                    const int i = i0 + lane;
                    const unsigned key = i < n ? bkey[i] : 0u;
                    const unsigned m = wave_umax_dpp(key);
                    if (m > bestk) {
                        bestk = m;
                        bi = i0 + __ffsll((long long)__ballot(key == m)) - 1;
                    }
                }
                if (bestk == 0u) break;
                const int bj = bent[bi];
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) {
                    aid[bj] = ~aid[bj];                 // claimed
                    bkey[bi] = 0u; bdone[bi] = 1;
                }
                __builtin_amdgcn_wave_barrier();
                for (int i0 = 0; i0 < n; i0 += 64) {
                    const int i = i0 + lane;
                    unsigned long long again = __ballot(i < n && bkey[i] != 0u && bent[i] == bj);
                    while (again) {
                        scan(i0 + __ffsll((long long)again) - 1);
                        again &= again - 1ull;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            // a box that claimed an entry inherits from it; the others open ids in decode order, at hits = 1 and at rest
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                const bool fresh = i < n && !bdone[i];
                const unsigned long long fm = __ballot(fresh);
                if (fresh) {
                    bid[i] = next_id + __popcll(fm & ((1ull << lane) - 1ull));
                    cgap[i] = -1; bhit[i] = 1; B[7 * tcap + i] = 0.0f; B[8 * tcap + i] = 0.0f;
                } else if (i < n) {
                    const int bj = bent[i];
                    const int my_gap = aage[bj];
                    const float evx = A[7 * tcap + bj], evy = A[8 * tcap + bj];
                    const float k = (float)(my_gap + 1);
                    const float ox = (B[i] - A[bj]) / k, oy = (B[tcap + i] - A[tcap + bj]) / k;
                    bid[i] = ~aid[bj]; cgap[i] = my_gap; bhit[i] = ahit[bj] + 1;
                    B[7 * tcap + i] = evx + gain * (ox - evx);
                    B[8 * tcap + i] = evy + gain * (oy - evy);
                }
                next_id += __popcll(fm);
            }
            __builtin_amdgcn_wave_barrier();
        } else
        for (int i = 0; i < n; ++i) {
            const float ax = B[i], ay = B[tcap + i], aw = B[2 * tcap + i], ah = B[3 * tcap + i], al = B[4 * tcap + i];
            unsigned bestk = 0u;
            int bj = 0;
            for (int j0 = 0; j0 < nt; j0 += 64) {          // 64 candidates per pass, as associate_kernel
                const int j = j0 + lane;
                unsigned key = 0u;
                if (j < nt && aid[j] >= 0 && aage[j] <= max_age && (ANY || A[4 * tcap + j] == al)) {
                    const float k = (float)(aage[j] + 1);
                    const float qx = A[j] + k * A[7 * tcap + j], qy = A[tcap + j] + k * A[8 * tcap + j];
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, qx, qy, A[2 * tcap + j], A[3 * tcap + j]);
                    if (iou >= thr) key = __float_as_uint(iou) + 1u;
                }
                const unsigned m = wave_umax_dpp(key);
                if (m > bestk) {
                    bestk = m;
                    bj = j0 + __ffsll((long long)__ballot(key == m)) - 1;
                }
            }
            int my_id, my_gap = -1, my_hits = 1;        // a new track: one frame with a box
            float nvx = 0.0f, nvy = 0.0f;               // ... and at rest
            if (bestk != 0u) {
                my_id = aid[bj];
                my_gap = aage[bj];
                my_hits = ahit[bj] + 1;
                const float evx = A[7 * tcap + bj], evy = A[8 * tcap + bj];
                const float k = (float)(my_gap + 1);
                const float ox = (ax - A[bj]) / k, oy = (ay - A[tcap + bj]) / k;
                nvx = evx + gain * (ox - evx);
                nvy = evy + gain * (oy - evy);
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) aid[bj] = -1;            // claimed
            } else {
                my_id = next_id++;
            }
            if (lane == 0) { bid[i] = my_id; cgap[i] = my_gap; bhit[i] = my_hits; B[7 * tcap + i] = nvx; B[8 * tcap + i] = nvy; }
            __builtin_amdgcn_wave_barrier();
        }
        for (int j = lane; j < cap; j += 64) {
            id[t * cap + j] = j < n ? bid[j] : -1;
            if (gp) gp[t * cap + j] = j < n ? cgap[j] : -1;
            if (hp) hp[t * cap + j] = j < n ? bhit[j] : -1;
        }
        // survivors, 64 entries per pass, compacted behind the frame's boxes by a wave scan
        int run = n;
        for (int j0 = 0; j0 < nt; j0 += 64) {
            const int j = j0 + lane;
            const bool surv = j < nt && aid[j] >= 0 && aage[j] < max_age;
            const unsigned long long bal = __ballot(surv);
            const int d = run + __popcll(bal & ((1ull << lane) - 1ull));
            if (surv && d < tcap) {
                B[d] = A[j]; B[tcap + d] = A[tcap + j]; B[2 * tcap + d] = A[2 * tcap + j]; B[3 * tcap + d] = A[3 * tcap + j];
                B[4 * tcap + d] = A[4 * tcap + j];
                bid[d] = aid[j];
                bage[d] = aage[j] + 1;
                B[7 * tcap + d] = A[7 * tcap + j]; B[8 * tcap + d] = A[8 * tcap + j];
                bhit[d] = ahit[j];
            }
            run += __popcll(bal);
        }
        nt = min(run, tcap); n0 = n;
        float *sw = A; A = B; B = sw;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (tk) readout(T - 1);
    if (lane == 0) nids[clip] = next_id;
    if constexpr (STREAM) {
        volatile int *aid = reinterpret_cast<volatile int *>(A + 5 * tcap), *aage = aid + tcap;
        volatile int *ahit = reinterpret_cast<volatile int *>(A + 9 * tcap);
        for (int j = lane; j < nt; j += 64) {
            float4 *q = reinterpret_cast<float4 *>(sb + j * DT_BOX_FLOATS);
            q[0] = make_float4(A[j], A[tcap + j], A[2 * tcap + j], A[3 * tcap + j]);
            q[1] = make_float4(0.0f, A[4 * tcap + j], 0.0f, 0.0f);
            si[j] = aid[j];
            sa[j] = aage[j];
            *reinterpret_cast<float2 *>(sv + j * 2) = make_float2(A[7 * tcap + j], A[8 * tcap + j]);
            sh[j] = ahit[j];
        }
        store_meta();
    }
}

// dynamic LDS of associate_tracks_kernel: none in the register form (tcap <= 64, T <= 64); general form: two tables of 10 words per entry
// and the frame's gaps.  The best-IoU-first order adds a 64-column key tile of the frame's boxes in the register form and three words
// per box in the general form.  More than 160 KB: launch_associate_tracks refuses the arguments.
size_t assoc_tracks_lds_bytes(int T, int cap, int tcap, int match)
{
    const bool best = (match & DT_MATCH_BEST_FIRST) != 0;
    if (tcap <= 64 && T <= 64) return best ? (size_t)64 * cap * sizeof(unsigned) : 0;      // the frame's keys, [cap][64]
    return ((size_t)20 * tcap + (best ? 4 : 1) * cap) * sizeof(float);                     // + key, entry, claimed per box
}

// one launch of associate_tracks_kernel<STREAM, MATCH>; the attribute is set once per device and instantiation
template <bool STREAM, int MATCH>
static int launch_associate_tracks_as(hipStream_t st, size_t lds, const float *boxes, const int *counts, int n_clips, int T, int cap, float thr,
                                      int max_age, int tcap, float gain, int min_hits, int *ids, int *nids, int *gaps, const TrackReadout &out,
                                      const AssocCarry &carry)
{
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(associate_tracks_kernel<STREAM, MATCH>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess;
        }))
        return 1;
    hipLaunchKernelGGL((associate_tracks_kernel<STREAM, MATCH>), dim3((unsigned)n_clips), dim3(64), lds, st, boxes, counts, T, cap, thr, max_age,
                       tcap, gain, min_hits, ids, nids, gaps, out, carry);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// 0: launched; 1: device error; 2: argument error (nothing launched).  carry.slots == null: the stateless launch.
// match: DT_MATCH_* bits, 0 = decode order within a label (the instantiation every call took before the bits existed).
int launch_associate_tracks(hipStream_t st, const float *boxes, const int *counts, int n_clips, int T, int cap, float thr,
                            int max_age, int tcap, float gain, int min_hits, int match, int *ids, int *nids, int *gaps,
                            const TrackReadout &out, const AssocCarry &carry)
{
    if (T <= 0 || cap <= 0 || tcap < cap || tcap > SM_COUNT_MASK || max_age < 0 || min_hits < 1) return 2;
    if (match < 0 || match > (DT_MATCH_BEST_FIRST | DT_MATCH_ANY_LABEL)) return 2;
    if (!(gain >= 0.0f && gain <= 1.0f)) return 2;      // (NaN fails both comparisons)
    if ((out.tracks != nullptr) != (out.tinfo != nullptr) || (out.tracks != nullptr) != (out.tcounts != nullptr)) return 2;
    const bool stream = carry.slots != nullptr;
    if (stream && (carry.tcap != tcap || !carry.vel || !carry.vstamp || !carry.hits || !carry.hstamp)) return 2;
    const size_t lds = assoc_tracks_lds_bytes(T, cap, tcap, match);
    if (lds > 160 * 1024) return 2;
    if (n_clips <= 0) return 0;
    const AssocCarry none{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
#define DT_TRACKS_LAUNCH(M)                                                                                                                  \
    case M:                                                                                                                                  \
        return stream ? launch_associate_tracks_as<true, M>(st, lds, boxes, counts, n_clips, T, cap, thr, max_age, tcap, gain, min_hits, ids, \
                                                            nids, gaps, out, carry)                                                          \
                      : launch_associate_tracks_as<false, M>(st, lds, boxes, counts, n_clips, T, cap, thr, max_age, tcap, gain, min_hits, ids, \
                                                             nids, gaps, out, none);
    switch (match) {
        DT_TRACKS_LAUNCH(0)
        DT_TRACKS_LAUNCH(1)
        DT_TRACKS_LAUNCH(2)
        DT_TRACKS_LAUNCH(3)
    }
#undef DT_TRACKS_LAUNCH
    return 2;
}

// ---------------------------------------------------------------------------
// highest-score box per frame (ties -> lowest index), one wavefront per frame
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void top_box_kernel(const float *boxes, const int *counts, int cap, float *out4)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = min(counts[f], cap);
    const float *b = boxes + (long long)f * cap * DT_BOX_FLOATS;
    float best = -1.0f;
    int bi = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const float s = b[i * 8 + 6];
        if (s > best) { best = s; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane < 4) out4[(long long)f * 4 + lane] = (n > 0) ? b[bi * 8 + lane] : 0.0f;
}

int launch_top_box(hipStream_t st, const float *boxes, const int *counts, int n_frames, int cap, float *out4)
{
    if (n_frames <= 0) return 0;
    hipLaunchKernelGGL(top_box_kernel, dim3((unsigned)n_frames), dim3(64), 0, st, boxes, counts, cap, out4);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------
// dt_boxes_map: decode's boxes, normalised to the network input, taken to a view's source frame
// ---------------------------------------------------------------------------
// One thread per (frame, row).  x' = x*ax + bx, y' = y*ay + by, w' = w*ax, h' = h*ay: the product is rounded, then the sum -- this
// file is built without FMA contraction.  The affines of a launch travel as kernel arguments; blockIdx.y picks the frame, so they are
// the same in every lane of a wave.  Rows from min(count, cap) on, and floats 4..7 of every row, are neither read nor written.
struct BoxesMapChunk { float a[BOXES_MAP_FRAMES_PER_LAUNCH][4]; };
static_assert(sizeof(BoxesMapChunk) + 2 * sizeof(void *) + sizeof(int) <= 4096, "a launch's affines and its other arguments fit HIP's 4096 bytes of kernel arguments");

__global__ __launch_bounds__(256) void boxes_map_kernel(BoxesMapChunk c, float *boxes, const int *counts, int cap)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    if (row >= min(counts[f], cap)) return;
    const float ax = c.a[f][0], bx = c.a[f][1], ay = c.a[f][2], by = c.a[f][3];
    float *b = boxes + ((long long)f * cap + row) * DT_BOX_FLOATS;
    const float x = b[0], y = b[1], w = b[2], h = b[3];
    b[0] = x * ax + bx;
    b[1] = y * ay + by;
    b[2] = w * ax;
    b[3] = h * ay;
}

int launch_boxes_map(hipStream_t st, float *boxes, const int *counts, int base, int count, int cap, const float *h_affine)
{
    if (count <= 0) return 0;
    if (count > BOXES_MAP_FRAMES_PER_LAUNCH || cap <= 0) return 2;
    BoxesMapChunk c;
    for (int j = 0; j < BOXES_MAP_FRAMES_PER_LAUNCH; ++j)
        for (int k = 0; k < 4; ++k) c.a[j][k] = h_affine[(size_t)(base + (j < count ? j : 0)) * 4 + k];
    dim3 grid((unsigned)((cap + 255) / 256), (unsigned)count);
    hipLaunchKernelGGL(boxes_map_kernel, grid, dim3(256), 0, st, c, boxes + (size_t)base * cap * DT_BOX_FLOATS, counts + base, cap);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
