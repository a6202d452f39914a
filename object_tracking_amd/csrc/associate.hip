// associate.hip -- the build-defined track-ID association (DESIGN.md "Track identity"): which box of a frame continues which
// track.  One wavefront per clip or stream slot.  Two kernels:
//   associate_kernel<STREAM>                    the previous-frame rule (dt_associate, dt_associate_stream); keeps no table
//   associate_table_kernel<STREAM, LEVEL, MATCH> the track table, at three levels: memory (ages), motion (+ velocities),
//                                                tracks (+ hit counts, the read-out and the match policies)
//
// This translation unit is compiled with -ffp-contract=off: the IoU and the velocity arithmetic restate numpy float32
// arithmetic op for op (tests/track_*_ref.py), which rounds after every multiply and add, so no fused multiply-add may be
// formed here.
#include "dt_internal.h"
#include <type_traits>

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
// Track identity with a TRACK TABLE (DESIGN.md "Track identity"): one kernel, three LEVELS.  Each level is the one below it plus
// the words it adds to an entry; everything a level does not have is under `if constexpr` and absent from its instances.
//
// ASSOC_MEMORY (max_age): a lost track keeps its id for up to max_age frames.  Per clip (or stream slot) a table of at most tcap
// entries -- box, label, id, age = frames since the track last had a box -- takes the place of "the previous frame": box i takes
// the id of the unclaimed entry of the same label with age <= max_age and the largest IoU >= thr (ties -> lowest table index),
// else opens a new id; gap = the claimed entry's age (-1: new id).  After the frame the table is rebuilt: the frame's boxes in
// decode order (age 0), behind them the unclaimed entries with age + 1 <= max_age in their previous order; the cut at tcap drops
// the tail.  With max_age = 0 the table is the previous frame and this is associate_kernel's rule bit for bit.  A claimed entry
// is marked by id = -1 (ids are >= 0).
//
// ASSOC_MOTION (motion gain): every entry is matched where a constant velocity predicts it.  An entry carries the velocity
// (vx, vy) of its box's x, y per frame.  With k = float(age + 1) the entry's PREDICTED box is (x + k*vx, y + k*vy, w, h) (one
// multiply, one add, each rounded: this file forms no FMA), and the IoU is taken against the predicted box.  When box i claims
// entry j: o = (x_i - x_j) / k on the STORED x_j (the correctly rounded quotient), v_i = v_j + gain * (o - v_j); a box that
// opens a new id starts at rest.  The rebuild carries the velocities along.  gain = 0 leaves every velocity 0 and gives the
// memory level's results bit for bit; the memory level itself takes the IoU against the stored x, y and divides nothing.
//
// ASSOC_TRACKS (track read-out): one more word per entry -- HITS, the frames in which the track had a box -- and the table written
// out once per frame.  A box that opens a new id starts at hits = 1, a box that claims entry j carries hits_j + 1, an unclaimed
// survivor keeps its hits; hits take no part in the match.  After frame t's rebuild (the cut at tcap included) the table is walked
// in table order and every CONFIRMED entry (hits >= min_hits) becomes one row of out.tracks / out.tinfo, compacted: x, y, w, h,
// label, vx, vy, 0 and id, age, hits, box.  An entry of age 0 reports its stored x, y; one of age a >= 1 reports x + float(a)*vx,
// y + float(a)*vy (one multiply, one add, each rounded).  Rows from the count on are written zero / -1: every row of the frame is
// written once.
//
// STREAM: the table continues in slot carry.slots[clip].  The slot's velocities (carry.vel) and hits (carry.hits) are the table's
// only while carry.vstamp[slot] / carry.hstamp[slot] equal the slot's association frame counter, which every association entry
// advances.  A level reads and writes the stamps of the words it has and no other: after a memory-level call (or associate_kernel)
// the table reads as at rest and at hits = 1 to the levels above, after a motion-level call as at hits = 1.
//
// MATCH (track match policy, ASSOC_TRACKS only): DT_MATCH_* bits chosen by the call.  ANY_LABEL drops the label comparison from the
// candidate test.  BEST_FIRST replaces the match block of each form: instead of the boxes in decode order, the candidate pair
// (box, entry) with the largest IoU key is taken repeatedly, ties to the lowest box, then the lowest entry; the boxes left over
// open their ids in decode order afterwards.  Load, rebuild, hits, read-out and store are shared by all four.
//
// ASSOC_MATCH_ASSIGN (dt_associate_tracks_assign, ASSOC_TRACKS only, never with BEST_FIRST): a third match block in each form.  The
// claimed pairs are an exact maximum-weight one-to-one assignment over the frame's candidates, weight = 1 + trunc(IoU * 2^20):
// dt_assign_max's method, orientation and tie rule (identity.hip:assign_max_kernel), step for step.  What the boxes inherit and the
// ids the others open are the best-first block's code behind the match.
//
// ASSOC_MATCH_SCORED (dt_associate_tracks_scored, beside ASSOC_MATCH_ASSIGN only; DESIGN.md "Track scores"): the assignment block runs
// twice per frame on masked weights.  Pass 0: the boxes whose score (float sc.at) is >= sc.high against the table, the assignment's own
// candidates.  Pass 1 (none with max_age_low = -1): the other boxes against the entries pass 0 left unclaimed, no older than
// min(max_age, max_age_low), at thr_low.  Both on the full [n][nt] shape, so orientation and tie rule are the assignment's.  An unclaimed
// box opens an id only with a score >= sc.fresh; any other is DROPPED (id -1, gap -1, hits 0) and leaves a DEAD row in the rebuilt table
// -- id -1, hits 0, age 0, at rest -- so that the leading rows stay the frame's boxes in decode order.  A dead row fails every candidate
// test (id >= 0, which also means "unclaimed"), is never confirmed (min_hits >= 1) and fails the survivor test at the next rebuild.
//
// One wavefront per clip, two forms like associate_kernel, chosen from tcap and T alone.
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

// a candidate's weight in the optimal assignment: 1 + the IoU in units of 2^-20, truncated (the product is exact: a power of two)
__device__ __forceinline__ int assign_weight(float iou) { return 1 + __float2int_rz(iou * (float)DT_ASSIGN_IOU_SCALE); }

template <bool STREAM, int LEVEL, int MATCH>
__global__ __launch_bounds__(64) void associate_table_kernel(const float *boxes, const int *counts, int T, int cap, float thr,
                                                             int max_age, int tcap, float gain, int min_hits, int *ids, int *nids,
                                                             int *gaps, TrackReadout out, AssocCarry carry,
                                                             std::conditional_t<(MATCH & ASSOC_MATCH_SCORED) != 0, AssocScore, AssocNoScore> sc)
{
    static_assert(LEVEL >= ASSOC_MEMORY && LEVEL <= ASSOC_TRACKS && (MATCH == 0 || LEVEL == ASSOC_TRACKS), "the match policies belong to the tracks level");
    constexpr bool VEL = LEVEL >= ASSOC_MOTION, HITS = LEVEL >= ASSOC_TRACKS;
    constexpr bool BEST = (MATCH & DT_MATCH_BEST_FIRST) != 0, ANY = (MATCH & DT_MATCH_ANY_LABEL) != 0;
    constexpr bool OPT = (MATCH & ASSOC_MATCH_ASSIGN) != 0;      // the optimal assignment; the launcher's bit, not a DT_MATCH_* one
    constexpr bool SCORED = (MATCH & ASSOC_MATCH_SCORED) != 0;   // the assignment in two passes by detection score; the launcher's bit too
    static_assert(!(BEST && OPT), "an assignment has no order");
    static_assert(!SCORED || OPT, "the scored passes are passes of the assignment");
    // the passes of a frame's assignment and what the second one matches at (SCORED only; every other instance has one pass and none of this)
    [[maybe_unused]] int n_pass = 1, low_age = 0;
    [[maybe_unused]] float low_thr = 0.0f;
    if constexpr (SCORED) {
        n_pass = sc.max_age_low < 0 ? 1 : 2;
        low_age = min(max_age, sc.max_age_low);
        low_thr = sc.thr_low;
    }
    constexpr int W = 7 + 2 * VEL + HITS;      // LDS words per entry of the general form: 5 box fields, id, age | vx, vy at 7, 8 | hits at 9
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int clip = blockIdx.x, lane = threadIdx.x;
    const float *bx = boxes + (long long)clip * T * cap * DT_BOX_FLOATS;
    const int *cnt = counts + (long long)clip * T;
    int *id = ids + (long long)clip * T * cap;
    int *gp = gaps ? gaps + (long long)clip * T * cap : nullptr;
    int *hp = nullptr;
    // the read-out of this clip: rows [T][tcap]; null = no read-out
    float *tk = nullptr;
    int *ti = nullptr, *tc = nullptr;
    if constexpr (HITS) {
        hp = out.hits ? out.hits + (long long)clip * T * cap : nullptr;
        tk = out.tracks ? out.tracks + (long long)clip * T * tcap * DT_TRACK_FLOATS : nullptr;
        ti = out.tracks ? out.tinfo + (long long)clip * T * tcap * DT_TRACK_INTS : nullptr;
        tc = out.tracks ? out.tcounts + (long long)clip * T : nullptr;
    }
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
        if constexpr (VEL) sv = carry.vel + (long long)slot * tcap * 2;
        if constexpr (HITS) sh = carry.hits + (long long)slot * tcap;
        sm = carry.meta + slot * STREAM_META;
        if constexpr (VEL) ss = carry.vstamp + slot;
        if constexpr (HITS) shs = carry.hstamp + slot;
        const int w = sm[SM_COUNT];
        n0 = min(w & SM_COUNT_MASK, cap);
        nt = min(n0 + (int)((unsigned)w >> SM_AGED_SHIFT), tcap);
        next_id = sm[SM_NEXT_ID];
        if constexpr (VEL) {
            const int f = sm[SM_ASSOC_FRAMES];
            const bool fok = f > 0 && f <= (1 << 30);
            vvalid = fok && *ss == f;
            if constexpr (HITS) hvalid = fok && *shs == f;
        }
    }
    auto store_meta = [&]() {
        if (lane == 0) {
            sm[SM_COUNT] = n0 | ((nt - n0) << SM_AGED_SHIFT);
            sm[SM_NEXT_ID] = next_id;
            const int f = sm[SM_ASSOC_FRAMES];
            const int f1 = f > (1 << 30) ? f : f + T;
            sm[SM_ASSOC_FRAMES] = f1;
            if constexpr (VEL) *ss = f1;                // (a saturated counter never validates: the test above)
            if constexpr (HITS) *shs = f1;
        }
    };
    // ---- register form (tcap <= 64, hence every frame <= 64 boxes; T <= 64) ----
    // Lane j holds table entry j (box, label, id, age; vx, vy and hits at the levels that have them) and box j of the current frame.
    // The match is associate_kernel's chain with `age <= max_age` in the eligibility test.  The table does not change within a
    // frame but for the claims, so lane j predicts its entry once per frame, in front of the chain over the boxes.  On a claim the
    // winner's stored x, y, age, vx, vy reach every lane by v_readlane at the wave-uniform bj and lane i selects its new velocity.
    // The rebuild is one ballot, one prefix count and seven (memory), nine (motion) or ten (tracks) ds_permute pushes: the kept
    // survivors go to lanes n .. n + kept - 1, every other lane to the lanes that are left, so the push is a permutation of the 64
    // lanes.  The read-out follows the rebuild: a ballot of the confirmed lanes, a popcount below the lane, and every lane writes
    // one row -- a confirmed lane its own, the others the empty rows behind the count.  Frame t + 1's boxes were requested at the
    // top of iteration t, in front of these stores, so the wait for them at the top of t + 1 does not wait for the read-out.
    if (tcap <= 64 && T <= 64) {
        const int cnt_l = lane < T ? min(cnt[lane], cap) : 0;
        [[maybe_unused]] float ns = 0.0f;               // SCORED: the score of the requested frame's box, fetched beside its label
        auto request = [&](int t, float4 &q, float &ql) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float *src = bx + ((long long)t * cap + (lane < n ? lane : 0)) * DT_BOX_FLOATS;
            q = *reinterpret_cast<const float4 *>(src);
            ql = src[5];
            if constexpr (SCORED) ns = src[sc.at];
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
                if constexpr (VEL) {
                    if (vvalid) {
                        const float2 w = *reinterpret_cast<const float2 *>(sv + lane * 2);
                        tvx = w.x; tvy = w.y;
                    }
                }
                if constexpr (HITS) thits = hvalid ? sh[lane] : 1;
            }
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int t = 0; t < T; ++t) {
            const int n = __builtin_amdgcn_readlane(cnt_l, t);
            const float cx = nq.x, cy = nq.y, cw = nq.z, ch = nq.w, cl = nl;        // waits for frame t's boxes
            [[maybe_unused]] const float cs = ns;
            if (t + 1 < T) request(t + 1, nq, nl);
            if (t > 0 && lane < cap) {
                id[(t - 1) * cap + lane] = outv;
                if (gp) gp[(t - 1) * cap + lane] = outg;
                if constexpr (HITS)
                    if (hp) hp[(t - 1) * cap + lane] = outh;
            }
            // the entry's predicted place in this frame; without velocities, where it is stored
            float qx = tbx, qy = tby;
            if constexpr (VEL) {
                const float tk_ = (float)(tage + 1);
                qx = tbx + tk_ * tvx; qy = tby + tk_ * tvy;
            }
            int cid = -1, cgap = -1, chits = -1;
            float cvx = 0.0f, cvy = 0.0f;
            if constexpr (BEST || OPT) {
                int tid0, cent;                         // the entries' ids before the claims mark them; lane = box: the entry it claimed
                if constexpr (OPT) {
                // optimal assignment (DESIGN.md "Track assignment"): dt_assign_max's method on the frame's weights, in registers.
                // The weights are an [n][ASSIGN_TILE_STRIDE] tile of dynamic LDS, row = box, column = lane = entry; the odd stride
                // spreads a column over the banks, for the transposed solve (nt < n) reads down one.  Solve rows and columns count
                // from 1 (assign_max_kernel): lane j - 1 owns column j's v, minv, way, used and p, lane i - 1 owns row i's u, and
                // the root column 0 is the wave-uniform j0 == 0 with p[0] = i.  `rin` marks the rows p[j] of the used columns
                // (lane = row), which are the rows a step adds delta to.  The arithmetic is assign_max_kernel's unsigned words.
                // Bounds: every loop below is counted (N rows, at most M + 1 steps, at most M + 1 flips), and every lane or tile
                // index comes from a ballot below M, from `way` (a j0 of the same range) or from p (i or a copy of a p), never from
                // a weight: non-finite boxes or a degenerate table may give unspecified ids, never an unbounded loop or an index
                // outside the tile.
                tid0 = tid; cent = -1;
                volatile int *wm = reinterpret_cast<volatile int *>(smem);
                volatile int *pent = wm + ASSIGN_TILE_STRIDE * cap, *pclm = pent + 64;   // the pairs: per box its entry, per entry whether claimed
                // SCORED: two passes over the one tile and the one solve.  Pass 0 weighs the HIGH boxes' rows (a NaN score is LOW) and leaves
                // the LOW rows zero; pass 1 weighs the LOW rows against the entries still live -- the claims of pass 0 have set tid = -1 --
                // and no older than low_age, at low_thr.  Both solve the full [n][nt] shape; the pairs of pass 0 stay in pent / pclm.
                [[maybe_unused]] unsigned long long hi = 0ull;
                if constexpr (SCORED) hi = __ballot(lane < n && cs >= sc.high);
                [[maybe_unused]] int pass = 0;
                do {
                const bool live = lane < nt && tid >= 0 && tage <= (SCORED && pass ? low_age : max_age);
                const float pthr = SCORED && pass ? low_thr : thr;
                [[maybe_unused]] const unsigned long long rows = SCORED && pass ? ~hi : hi;
                for (int i = 0; i < n; ++i) {
                    const float ax = readlane_f(cx, i), ay = readlane_f(cy, i), aw = readlane_f(cw, i), ah = readlane_f(ch, i);
                    const float al = readlane_f(cl, i);
                    const float iou = bbox_iou_ref(ax, ay, aw, ah, qx, qy, tbw, tbh);
                    wm[i * ASSIGN_TILE_STRIDE + lane] = (live && (!SCORED || ((rows >> i) & 1ull)) && (ANY || tbl == al) && iou >= pthr) ? assign_weight(iou) : 0;
                }
                if (!SCORED || pass == 0) { pent[lane] = -1; pclm[lane] = 0; }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                const bool tr = nt < n;                 // the solve's rows are the entries
                const int N = tr ? nt : n, M = tr ? n : nt;
                unsigned zu = 0u, zv = 0u;
                int zp = 0, zway = 0;
                for (int i = 1; i <= N; ++i) {
                    unsigned minv = (unsigned)ASSIGN_INF;
                    bool used = false, rin = false;
                    int j0 = 0, i0 = i;
                    bool reached = false;
                    for (int step = 0; step <= M; ++step) {
                        rin = rin || lane == i0 - 1;
                        const unsigned ui = (unsigned)__builtin_amdgcn_readlane((int)zu, i0 - 1);
                        const bool act = lane < M && !used;
                        unsigned key = 0u;
                        if (act) {
                            const int wt = tr ? wm[lane * ASSIGN_TILE_STRIDE + (i0 - 1)] : wm[(i0 - 1) * ASSIGN_TILE_STRIDE + lane];
                            const unsigned cur = 0u - (unsigned)wt - ui - zv;
                            if ((int)cur < (int)minv) { minv = cur; zway = j0; }
                            key = (unsigned)ASSIGN_INF - minv;
                        }
                        const unsigned top = wave_umax_dpp(key);
                        const unsigned long long bal = __ballot(act && key == top);
                        if (!bal) break;                // no unused column: cannot happen while N <= M
                        const int j1 = __ffsll((long long)bal);
                        const unsigned delta = (unsigned)ASSIGN_INF - top;
                        if (rin) zu += delta;
                        if (used) zv -= delta; else minv -= delta;
                        j0 = j1;
                        used = used || lane == j1 - 1;
                        i0 = __builtin_amdgcn_readlane(zp, j1 - 1);
                        if (i0 == 0) { reached = true; break; }
                    }
                    // flip the path back to the root
                    for (int step = 0; reached && step <= M && j0 != 0; ++step) {
                        const int jp = __builtin_amdgcn_readlane(zway, j0 - 1);
                        const int pn = jp == 0 ? i : __builtin_amdgcn_readlane(zp, (jp - 1) & 63);
                        zp = lane == j0 - 1 ? pn : zp;
                        j0 = jp;
                    }
                }
                // lane = column: its pair, unless the pair has no weight
                if (lane < M && zp >= 1) {
                    const int b = tr ? lane : zp - 1, e = tr ? zp - 1 : lane;
                    if (wm[b * ASSIGN_TILE_STRIDE + e] != 0) { pent[b] = e; pclm[e] = 1; }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                cent = pent[lane];
                if (pclm[lane]) tid = -1;               // claimed
                __builtin_amdgcn_wave_barrier();        // the next tile (the second pass's, the next frame's) stands behind these reads
                } while (SCORED && ++pass < n_pass);
                } else {
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
                cent = -1; tid0 = tid;
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
                bool fresh = lane < n && cent < 0;
                if constexpr (SCORED) {
                    // ... those of them with a score >= sc.fresh.  The others are DROPPED: id -1, gap -1, hits 0, at rest, and the rebuild
                    // below makes of them a dead row, which no candidate test accepts (tid >= 0) and no survivor test keeps
                    if (fresh && !(cs >= sc.fresh)) { fresh = false; chits = 0; }
                }
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
                    if constexpr (HITS) my_hits = __builtin_amdgcn_readlane(thits, bj) + 1;
                    if constexpr (VEL) {
                        const float ex = readlane_f(tbx, bj), ey = readlane_f(tby, bj);
                        const float evx = readlane_f(tvx, bj), evy = readlane_f(tvy, bj);
                        const float k = (float)(my_gap + 1);
                        const float ox = (ax - ex) / k, oy = (ay - ey) / k;
                        nvx = evx + gain * (ox - evx);
                        nvy = evy + gain * (oy - evy);
                    }
                    tid = lane == bj ? -1 : tid;        // claimed
                } else {
                    my_id = next_id++;
                }
                cid = lane == i ? my_id : cid;
                cgap = lane == i ? my_gap : cgap;
                if constexpr (HITS) chits = lane == i ? my_hits : chits;
                if constexpr (VEL) {
                    cvx = lane == i ? nvx : cvx;
                    cvy = lane == i ? nvy : cvy;
                }
            }
            outv = cid; outg = cgap; outh = chits;      // lanes >= n keep -1
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
            float pvx = 0.0f, pvy = 0.0f;
            if constexpr (VEL) {
                pvx = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tvx)));
                pvy = __int_as_float(__builtin_amdgcn_ds_permute(da, __float_as_int(tvy)));
            }
            const int pi = __builtin_amdgcn_ds_permute(da, tid);
            const int pa = __builtin_amdgcn_ds_permute(da, tage);
            int phit = 0;
            if constexpr (HITS) phit = __builtin_amdgcn_ds_permute(da, thits);
            const bool cur = lane < n;
            tbx = cur ? cx : px; tby = cur ? cy : py; tbw = cur ? cw : pw; tbh = cur ? ch : ph; tbl = cur ? cl : pl;
            if constexpr (VEL) { tvx = cur ? cvx : pvx; tvy = cur ? cvy : pvy; }
            tid = cur ? cid : pi;
            tage = cur ? 0 : pa + 1;
            if constexpr (HITS) thits = cur ? chits : phit;
            nt = n + kept; n0 = n;      // lanes >= nt hold whatever the permutation left there: don't-care, every use is guarded by `lane < nt`
            // read-out of the table as it now stands; lane = table index, so an age-0 entry's box index is the lane
            if constexpr (HITS) if (tk) {
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
            if constexpr (HITS)
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
                if constexpr (VEL) *reinterpret_cast<float2 *>(sv + lane * 2) = make_float2(tvx, tvy);
                if constexpr (HITS) sh[lane] = thits;
            }
            store_meta();
        }
        return;
    }
    // ---- general form (any tcap): two tables of W words per entry in LDS, read and rebuilt in turn; the current frame's boxes are loaded
    // straight into the leading entries of the table under construction, where the rebuild wants them ----
    const int TS = W * tcap;                             // one table: [5][tcap] box fields | [tcap] ids | [tcap] ages | VEL: [2][tcap] vx, vy | HITS: [tcap] hits
    float *A = smem, *B = smem + TS;
    volatile int *cgap = reinterpret_cast<volatile int *>(smem + 2 * TS);      // [cap] gaps of the current frame
    // best-IoU-first order only: per box its best remaining candidate (key, entry) and whether it has claimed one, [cap] each
    volatile unsigned *bkey = reinterpret_cast<volatile unsigned *>(smem + 2 * TS + cap);
    volatile int *bent = reinterpret_cast<volatile int *>(smem + 2 * TS + 2 * cap);
    volatile int *bdone = reinterpret_cast<volatile int *>(smem + 2 * TS + 3 * cap);
    // SCORED only: the current frame's scores, [cap], behind the assignment's six work arrays
    [[maybe_unused]] volatile float *bsc = reinterpret_cast<volatile float *>(smem + 2 * TS + 4 * cap + 6 * (tcap + 1));
    // read-out of table A (nt entries, as frame t left it): 64 entries per pass compacted by a running count, the way the survivor
    // pass compacts; then the empty rows behind the count.  Called once the NEXT frame's boxes have been fetched (below), so these
    // stores stand behind those loads and never in front of them.  (HITS only: no other level calls it.)
    [[maybe_unused]] auto readout = [&](int t) {
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
            if constexpr (VEL) {
                A[7 * tcap + j] = vvalid ? sv[2 * j] : 0.0f;
                A[8 * tcap + j] = vvalid ? sv[2 * j + 1] : 0.0f;
            }
            if constexpr (HITS) ahit[j] = hvalid ? sh[j] : 1;
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
            if constexpr (BEST || OPT) bdone[j] = 0;
            if constexpr (SCORED) bsc[j] = q[sc.at];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if constexpr (HITS)
            if (tk && t > 0) readout(t - 1);              // table A is frame t-1's until the first claim below
        if constexpr (BEST || OPT) {
            if constexpr (OPT) {
            // optimal assignment (DESIGN.md "Track assignment"): assign_max_kernel's loop with its six work arrays of tcap + 1 words
            // behind the per-box words, on the frame's weights.  No n x nt matrix is held: a weight is recomputed from table A and the
            // frame's boxes (in B) wherever the solver reads one -- a pure function of both, neither of which changes before the
            // claims below, so its bits repeat.  Solve rows and columns count from 1 and column 0 is the root; the solve is
            // transposed (rows = entries) when nt < n.  Bounds as in the register form: every loop is counted, and every index into
            // the tables or the work arrays is a counter, a ballot position below M, a `way` (a j0) or a p (i or a copy of a p),
            // never a weight: non-finite boxes or a degenerate table may give unspecified ids, never an unbounded loop or an index
            // outside the LDS.
            const int L = tcap + 1;
            volatile unsigned *zu = reinterpret_cast<volatile unsigned *>(smem + 2 * TS + 4 * cap), *zv = zu + L, *zminv = zv + L;
            volatile int *zway = reinterpret_cast<volatile int *>(zminv + L), *zp = zway + L, *zused = zp + L;
            // SCORED: two passes of the one solve, the six work arrays initialised anew by each.  Pass 0 weighs the HIGH boxes (a NaN score
            // is LOW), pass 1 the LOW ones against the entries no older than low_age, at low_thr; the entries pass 0 claimed have a
            // complemented id by then, so `aid[e] >= 0` is "live and unclaimed" in both.  The pairs of pass 0 stay in bent / bdone.
            [[maybe_unused]] int pass = 0;
            do {
            // an id below 0 is a claimed entry or a dead row (one a scored call left in the slot): no candidate of any box
            auto weight_of = [&](int b, int e) -> int {       // box b of the frame, entry e of table A
                if constexpr (SCORED) {
                    if ((bsc[b] >= sc.high) == (pass != 0)) return 0;
                }
                const int page = SCORED && pass ? low_age : max_age;
                const float pthr = SCORED && pass ? low_thr : thr;
                if (!(aid[e] >= 0 && aage[e] <= page && (ANY || A[4 * tcap + e] == B[4 * tcap + b]))) return 0;
                const float k = (float)(aage[e] + 1);
                const float qx = A[e] + k * A[7 * tcap + e], qy = A[tcap + e] + k * A[8 * tcap + e];
                const float iou = bbox_iou_ref(B[b], B[tcap + b], B[2 * tcap + b], B[3 * tcap + b], qx, qy, A[2 * tcap + e], A[3 * tcap + e]);
                return iou >= pthr ? assign_weight(iou) : 0;
            };
            const bool tr = nt < n;                     // the solve's rows are the entries
            const int N = tr ? nt : n, M = tr ? n : nt;
            auto weight = [&](int i, int j) { return tr ? weight_of(j - 1, i - 1) : weight_of(i - 1, j - 1); };
            for (int j = lane; j <= M; j += 64) { zv[j] = 0u; zp[j] = 0; zway[j] = 0; }
            for (int i = lane; i <= N; i += 64) zu[i] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            for (int i = 1; i <= N; ++i) {
                for (int j = lane; j <= M; j += 64) { zminv[j] = (unsigned)ASSIGN_INF; zused[j] = 0; }
                if (lane == 0) zp[0] = i;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                int j0 = 0;
                bool reached = false;
                for (int step = 0; step <= M; ++step) {
                    if (lane == 0) zused[j0] = 1;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    const int i0 = min(max(zp[j0], 1), N);     // (in 1..N by construction; the clamp keeps the table index there whatever happens)
                    const unsigned ui = zu[i0];
                    unsigned bestk = 0u;
                    int j1 = -1;
                    for (int jb = 1; jb <= M; jb += 64) {
                        const int j = jb + lane;
                        const bool act = j <= M && zused[j] == 0;
                        unsigned key = 0u;
                        if (act) {
                            const unsigned cur = 0u - (unsigned)weight(i0, j) - ui - zv[j];
                            unsigned m = zminv[j];
                            if ((int)cur < (int)m) { m = cur; zminv[j] = cur; zway[j] = j0; }
                            key = (unsigned)ASSIGN_INF - m;
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
                    if (j1 < 0) break;                  // no unused column: cannot happen while N <= M
                    const unsigned delta = (unsigned)ASSIGN_INF - bestk;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    for (int j = lane; j <= M; j += 64) {
                        if (zused[j]) {                 // p is one-to-one on the used columns
                            const int pj = min(max(zp[j], 0), N);
                            zu[pj] = zu[pj] + delta;
                            zv[j] = zv[j] - delta;
                        } else {
                            zminv[j] = zminv[j] - delta;
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    j0 = j1;
                    if (zp[j0] == 0) { reached = true; break; }
                }
                // flip the path back to the root
                if (lane == 0 && reached) {
                    int j = j0;
                    for (int step = 0; step <= M && j != 0; ++step) {
                        const int jp = min(max(zway[j], 0), M);
                        zp[j] = zp[jp];
                        j = jp;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
            // the pairs that have a weight: the box notes its entry, the entry is marked like a best-first claim (complemented id)
            for (int j = 1 + lane; j <= M; j += 64) {
                const int i = zp[j];
                if (i < 1 || i > N) continue;
                const int b = tr ? j - 1 : i - 1, e = tr ? i - 1 : j - 1;
                if (weight_of(b, e) == 0) continue;
                bent[b] = e; bdone[b] = 1;
                aid[e] = ~aid[e];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            } while (SCORED && ++pass < n_pass);
            } else {
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
            }
            // a box that claimed an entry inherits from it; the others open ids in decode order, at hits = 1 and at rest
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                bool fresh = i < n && !bdone[i];
                [[maybe_unused]] bool drop = false;
                if constexpr (SCORED) {
                    // ... those of them with a score >= sc.fresh.  The others are DROPPED and leave a dead row: id -1, hits 0, at rest
                    drop = fresh && !(bsc[i] >= sc.fresh);
                    fresh = fresh && !drop;
                }
                const unsigned long long fm = __ballot(fresh);
                if (fresh) {
                    bid[i] = next_id + __popcll(fm & ((1ull << lane) - 1ull));
                    cgap[i] = -1; bhit[i] = 1; B[7 * tcap + i] = 0.0f; B[8 * tcap + i] = 0.0f;
                } else if (SCORED && drop) {
                    bid[i] = -1; cgap[i] = -1; bhit[i] = 0; B[7 * tcap + i] = 0.0f; B[8 * tcap + i] = 0.0f;
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
                    float qx = A[j], qy = A[tcap + j];
                    if constexpr (VEL) {
                        const float k = (float)(aage[j] + 1);
                        qx = A[j] + k * A[7 * tcap + j]; qy = A[tcap + j] + k * A[8 * tcap + j];
                    }
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
                if constexpr (HITS) my_hits = ahit[bj] + 1;
                if constexpr (VEL) {
                    const float evx = A[7 * tcap + bj], evy = A[8 * tcap + bj];
                    const float k = (float)(my_gap + 1);
                    const float ox = (ax - A[bj]) / k, oy = (ay - A[tcap + bj]) / k;
                    nvx = evx + gain * (ox - evx);
                    nvy = evy + gain * (oy - evy);
                }
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) aid[bj] = -1;            // claimed
            } else {
                my_id = next_id++;
            }
            if (lane == 0) {
                bid[i] = my_id; cgap[i] = my_gap;
                if constexpr (HITS) bhit[i] = my_hits;
                if constexpr (VEL) { B[7 * tcap + i] = nvx; B[8 * tcap + i] = nvy; }
            }
            __builtin_amdgcn_wave_barrier();
        }
        for (int j = lane; j < cap; j += 64) {
            id[t * cap + j] = j < n ? bid[j] : -1;
            if (gp) gp[t * cap + j] = j < n ? cgap[j] : -1;
            if constexpr (HITS)
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
                if constexpr (VEL) { B[7 * tcap + d] = A[7 * tcap + j]; B[8 * tcap + d] = A[8 * tcap + j]; }
                if constexpr (HITS) bhit[d] = ahit[j];
            }
            run += __popcll(bal);
        }
        nt = min(run, tcap); n0 = n;
        float *sw = A; A = B; B = sw;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (HITS)
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
            if constexpr (VEL) *reinterpret_cast<float2 *>(sv + j * 2) = make_float2(A[7 * tcap + j], A[8 * tcap + j]);
            if constexpr (HITS) sh[j] = ahit[j];
        }
        store_meta();
    }
}


size_t assoc_table_lds_bytes(int level, int T, int cap, int tcap, int match)
{
    const bool best = (match & DT_MATCH_BEST_FIRST) != 0, opt = (match & ASSOC_MATCH_ASSIGN) != 0;
    if (tcap <= 64 && T <= 64) {
        if (opt) return ((size_t)ASSIGN_TILE_STRIDE * cap + 128) * sizeof(int);            // the frame's weights, [cap][65], and the pairs
        return best ? (size_t)64 * cap * sizeof(unsigned) : 0;                             // the frame's keys, [cap][64]
    }
    const int words = 7 + 2 * (level >= ASSOC_MOTION) + (level >= ASSOC_TRACKS);           // per entry, as the kernel's W
    const bool scored = (match & ASSOC_MATCH_SCORED) != 0;                                 // (the register form above needs no word for it)
    return ((size_t)2 * words * tcap + ((best || opt ? 4 : 1) + scored) * cap              // + key, entry, claimed per box; scored: + its score
            + (opt ? (size_t)6 * (tcap + 1) : 0)) * sizeof(float);                         // + the solver's u, v, minv, way, p, used
}

// one launch of associate_table_kernel<STREAM, LEVEL, MATCH>; the attribute is set once per device and instantiation
template <bool STREAM, int LEVEL, int MATCH>
static int launch_table_as(hipStream_t st, size_t lds, const AssocTableArgs &a, int n_clips)
{
    static PerDeviceOnce attr;
    if (attr.ensure(nullptr, [](int) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(associate_table_kernel<STREAM, LEVEL, MATCH>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess;
        }))
        return 1;
    std::conditional_t<(MATCH & ASSOC_MATCH_SCORED) != 0, AssocScore, AssocNoScore> sc{};
    if constexpr ((MATCH & ASSOC_MATCH_SCORED) != 0) sc = a.score;
    hipLaunchKernelGGL((associate_table_kernel<STREAM, LEVEL, MATCH>), dim3((unsigned)n_clips), dim3(64), lds, st, a.boxes, a.counts, a.T, a.cap,
                       a.thr, a.max_age, a.tcap, a.gain, a.min_hits, a.ids, a.nids, a.gaps, a.out, a.carry, sc);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_associate_table(hipStream_t st, const AssocTableArgs &a, int n_clips)
{
    if (a.level < ASSOC_MEMORY || a.level > ASSOC_TRACKS) return 2;
    // the memory and motion entries have always accepted an empty call before looking at its shape; the tracks entries look first
    if (n_clips <= 0 && a.level < ASSOC_TRACKS) return 0;
    if (a.T <= 0 || a.cap <= 0 || a.tcap < a.cap || a.tcap > SM_COUNT_MASK || a.max_age < 0) return 2;
    if (a.level >= ASSOC_MOTION && !(a.gain >= 0.0f && a.gain <= 1.0f)) return 2;      // (NaN fails both comparisons)
    if (a.level < ASSOC_TRACKS ? a.match != 0 : (a.match < 0 || a.match > (DT_MATCH_BEST_FIRST | DT_MATCH_ANY_LABEL))) return 2;
    if (a.assign && (a.level != ASSOC_TRACKS || (a.match & DT_MATCH_BEST_FIRST))) return 2;
    if (a.scored) {
        const AssocScore &s = a.score;
        if (!a.assign || s.at < 0 || s.at >= DT_BOX_FLOATS || s.max_age_low < -1) return 2;
        if (s.high != s.high || s.fresh != s.fresh || s.thr_low != s.thr_low) return 2;      // a NaN
    }
    const int match = assoc_kernel_match(a);
    if (a.level == ASSOC_TRACKS) {
        const TrackReadout &o = a.out;
        if (a.min_hits < 1) return 2;
        if ((o.tracks != nullptr) != (o.tinfo != nullptr) || (o.tracks != nullptr) != (o.tcounts != nullptr)) return 2;
    }
    const AssocCarry &c = a.carry;
    const bool stream = c.slots != nullptr;
    if (stream && c.tcap != a.tcap) return 2;
    if (stream && a.level >= ASSOC_MOTION && (!c.vel || !c.vstamp)) return 2;
    if (stream && a.level >= ASSOC_TRACKS && (!c.hits || !c.hstamp)) return 2;
    const size_t lds = assoc_table_lds_bytes(a.level, a.T, a.cap, a.tcap, match);
    if (lds > 160 * 1024) return 2;
    if (n_clips <= 0) return 0;
#define DT_TABLE_LAUNCH(L, M) \
    case (L) * 16 + (M): return stream ? launch_table_as<true, L, M>(st, lds, a, n_clips) : launch_table_as<false, L, M>(st, lds, a, n_clips);
    switch (a.level * 16 + match) {
        DT_TABLE_LAUNCH(ASSOC_MEMORY, 0)
        DT_TABLE_LAUNCH(ASSOC_MOTION, 0)
        DT_TABLE_LAUNCH(ASSOC_TRACKS, 0)
        DT_TABLE_LAUNCH(ASSOC_TRACKS, 1)
        DT_TABLE_LAUNCH(ASSOC_TRACKS, 2)
        DT_TABLE_LAUNCH(ASSOC_TRACKS, 3)
        DT_TABLE_LAUNCH(ASSOC_TRACKS, ASSOC_MATCH_ASSIGN)
        DT_TABLE_LAUNCH(ASSOC_TRACKS, ASSOC_MATCH_ASSIGN | DT_MATCH_ANY_LABEL)
        DT_TABLE_LAUNCH(ASSOC_TRACKS, ASSOC_MATCH_SCORED | ASSOC_MATCH_ASSIGN)
        DT_TABLE_LAUNCH(ASSOC_TRACKS, ASSOC_MATCH_SCORED | ASSOC_MATCH_ASSIGN | DT_MATCH_ANY_LABEL)
    }
#undef DT_TABLE_LAUNCH
    return 2;
}
