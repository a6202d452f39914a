// Internal declarations shared by the HIP translation units of libmi355_dt.so.
// gfx950 (MI355X, CDNA4) only -- no other target is supported or compiled.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mi355_dt.h"

// One-time, PER-DEVICE set-up of a launch site (hipFuncSetAttribute for large dynamic LDS, small constant buffers):
// kernel attributes and allocations belong to a device, so a process that drives several GPUs must repeat them on
// each.  `ensure(&dev, setup)` runs `setup(dev)` once per device, serialised by a mutex, and hands the calling thread's
// device id back to the CALLER (nothing device-specific is kept in shared state, so two host threads on different
// devices cannot see each other's id).  It returns non-zero -- the caller fails its launch -- when the set-up failed,
// the device cannot be determined, or it lies beyond the 64 devices tracked (never aliased onto device 0).
struct PerDeviceOnce {
    std::atomic<unsigned long long> mask{0};
    std::mutex mu;
    template <class F> int ensure(int *dev_out, F &&setup)
    {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return 1;
        if (dev_out) *dev_out = dev;
        if ((mask.load(std::memory_order_acquire) >> dev) & 1ull) return 0;
        std::lock_guard<std::mutex> lk(mu);
        if ((mask.load(std::memory_order_acquire) >> dev) & 1ull) return 0;
        const int rc = setup(dev);
        if (rc == 0) mask.fetch_or(1ull << dev, std::memory_order_release);
        return rc;
    }
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------
// implicit-GEMM convolution (conv_igemm.hip)
// ---------------------------------------------------------------------------
enum { ORD_LINEAR = 0, ORD_QUAD = 1 };
enum { EPI_PLAIN = 0, EPI_POOL = 1, EPI_POOL_BOTH = 2, EPI_S2D = 3, EPI_GATES = 4, EPI_PARTIAL = 5 };

struct ConvArgs {
    // input activation: pixel (b,h,w) at in + b*in_bs + (h*W+w)*in_ld, Cin floats read
    const float *in;
    long long in_bs;
    int in_ld;
    // packed weights [Npad][K], k = ((ci/32)*taps + tap)*32 + ci%32 (k contiguous); bias [Npad] or null
    const float *wt;
    const float *bias;
    // primary output (dense unless EPI_GATES): row r at out + r*out_ld (+ col)
    float *out;
    long long out_bs;
    int out_ld;
    // secondary output: pooled tensor for EPI_POOL_BOTH
    float *out2;
    int out2_ld;
    // EPI_GATES: z = acc + xproj; c updated in place; h written to out
    const float *xproj;
    long long xp_bs;
    int xp_ld;
    float *cstate;
    long long c_bs;
    int c_ld;
    int B, H, W, Cin, N, M, K;
    int npad;     // rows of wt that exist (0 = N rounded up to 128); 256-wide column tiles need N rounded up to 256
    float slope;  // LeakyReLU slope; 1.0f = linear
    int act;      // 0: LeakyReLU(slope), 1: sigmoid (Dense heads)
    const float *zeros; // >= 16 B of device zeros: source of out-of-image taps (set by launch_conv_igemm)
    int ksplit;    // EPI_PARTIAL: number of K splits (grid.y); out = slab [ksplit][M][out_ld]
    int tile_gn;   // column tiles per group in the tile order (0 = all; set by launch_conv_igemm)
    // batched GEMMs (Winograd positions): zbatch problems of ntiles tiles each share ONE linear tile index (tile t belongs to problem
    // z = t / ntiles); problem z reads in + z*z_in, wt + z*z_wt and writes out + z*z_out (floats)
    int zbatch;
    long long z_in, z_wt, z_out;
    int force_cfg; // > 0: tile configuration + 1 forced by the caller's policy (Policy::conv_cfg); 0: none
    unsigned *amax_out; // EPI_PLAIN (no split-K) / EPI_POOL / EPI_S2D: non-null = max |x| of the stored outputs into this slot (dt_amax_publish)
    int wg_cap;    // test only (dt_conv_igemm), 0 in production -- like WinoArgs::wg_cap: > 0 = a persistent launch uses at most this many workgroups
};

// Tile configurations of the MFMA kernel
enum { CFG_128x128 = 0, CFG_128x64 = 1, CFG_256x128 = 2, CFG_256x256 = 3, CFG_64x128 = 4 };

// What launch_conv_igemm does with a call (plan_conv_igemm): rc 0 = launches, 2 = refuses the arguments; the tile configuration that runs
// (after a forced one, the 256x256 -> 256x128 fallback and the gate / split-K instances' own tiles), its tile and workgroup shape,
// whether the instance is the persistent one, and the grid over `total` tiles.
struct ConvPlan {
    int rc, cfg, bm, bn, wgm, wgn, threads, persist, grid_x, grid_y, total;
};
ConvPlan plan_conv_igemm(const ConvArgs &a, int ks, int order, int epi, int cfg);
int launch_conv_igemm(hipStream_t st, const ConvArgs &a, int ks, int order, int epi, int cfg);
int launch_splitk_reduce(hipStream_t st, const float *slab, int S, long long M, int N, const float *bias, float slope,
                         float *out, int out_ld);

// host-side packing: Keras HWIO kernel -> [npad][ks*ks*cin_dst], k contiguous in the kernel's chunk order.
//   cin_map[cin_dst]: source input channel or -1 (zero);  n_map[npad]: source
//   output channel or -1 (zero row);  scale[cout_src] multiplies each output
//   channel (folded BatchNorm) or null.
void pack_conv_weights(const float *hwio, int ks, int cin_src, int cout_src, const int *cin_map,
                       int cin_dst, const int *n_map, int npad, const float *scale, float *dst);

// ---------------------------------------------------------------------------
// Winograd F(2x2,3x3) transforms around the batched MFMA GEMM (winograd.hip)
// ---------------------------------------------------------------------------
struct WinoArgs {
    // geometry: B images of H x W; th x tw tiles of ts x ts outputs per image (ts = 2 or 4); Mt = B*th*tw;
    // P = (ts+2)^2 Winograd positions
    int B, H, W, th, tw, Mt, ts;
    int g;   // frames per side of the virtual mosaic the tiles live on (1: one frame; winograd.hip:vpixel)
    int ph, pw;   // g > 1: the mosaic's frame pitch, rows / columns from one frame's origin to the next (>= H + 1 / W + 1: at least one separator of zeros;
                  // EVEN where out2 is set, so that no 2x2 pooling window straddles a tile or a frame -- network.hip:wino_geometry)
    // input transform: in (NHWC, pixel stride in_ld, image stride in_bs), C channels -> v [P][Mt][C]
    const float *in;
    long long in_bs;
    int in_ld, C;
    float *v;
    unsigned short *v_s3;   // non-null: V as three bf16 terms [P][3][C/16][Mp][16] for wino_gemm_s3.hip instead of v (ts == 6, C % 32 == 0)
    int Mp;                 // rows of that layout (Mt rounded up to the GEMM's row tile)
    int nt;                 // 2: v_s3 takes TWO fp16 terms [P][2][C/16][Mp][16] of the scaled V (wino_gemm_s3.hip's fp16 form); 0 / 3: three bf16 terms
    const unsigned *amax;   // nt = 2: the max-|x| slot (DT_AMAX_SUB words) of the input tensor
    unsigned *amax_out;     // output transform (plain epilogue, thread-per-item kernels): non-null = take max |x| over the values STORED to out2 if it is set,
                            // else to out, into this slot (dt_amax_publish); the caller zeroes the slot
    // output transform: m [P][Mt][m_ld], N columns -> out (full resolution, may be null) / out2 (2x2 pooled, may be null)
    const float *m;
    int m_ld, N;
    const float *bias;
    const float *bias16;    // non-null (plain epilogue, slope 1): a CORRECTION to `bias` for pixels on the image border, [16][N] indexed by
                            // (h == 0) | (h == H - 1) << 1 | (w == 0) << 2 | (w == W - 1) << 3 (entry 0 unused: interior pixels take `bias` alone) -- the
                            // merged ConvLSTM input projection: conv_23's bias reaches the projection through the taps that lie inside the image only
    float slope;
    float *out;
    long long out_bs;
    int out_ld;
    float *out2;
    int out2_ld;
    // gate variant (ConvLSTM2D): xproj / cstate as in ConvArgs
    const float *xproj;
    long long xp_bs;
    int xp_ld;
    float *cstate;
    long long c_bs;
    int c_ld;
    // test only (dt_wino_input / dt_wino_output), both 0 in production -- like ConvArgs::force_cfg
    int force_form;         // fp32 F(6x6), where two kernels exist for the same arguments: 1 = the thread-per-item kernel, 2 = the lane-cooperative one
    int wg_cap;             // > 0: at most this many workgroups, on top of the launcher's own cap (the grid-stride loops at small shapes)
};
// Which kernel a transform launch takes and with what grid: decided by choose_wino_input / choose_wino_output (winograd.hip; pure: no launch), the one
// place launch_wino_input / launch_wino_output switch on.  form 0 = the arguments are refused (the launchers return 2).
enum { WIN_TPI2 = 1,     // wino_input_kernel<2,4>
       WIN_TPI4,         // wino_input_kernel<4,4>
       WIN_TPI6,         // wino_input_kernel<6,2>
       WIN_TPI4_S3,      // wino_input_kernel<4,4,true>: three bf16 terms, C % 32 != 0
       WIN_COOP6,        // wino_input_coop6_kernel
       WIN_S3_6,         // wino_input_s3_kernel<6>
       WIN_S3_4,         // wino_input_s3_kernel<4>
       WIN_H2_6,         // wino_input_s3_kernel<6,2>
       WIN_H2_4 };       // wino_input_s3_kernel<4,2>
enum { WOUT_TPI6 = 1,    // wino_output_kernel<6,2>
       WOUT_TPI4,        // wino_output_kernel<4,2>
       WOUT_TPI2,        // wino_output_kernel<2,4>
       WOUT_COOP6,       // wino_output_coop6_kernel
       WOUT_GATES6,      // wino_output_gates_kernel<6,1>
       WOUT_GATES4,      // wino_output_gates_kernel<4,1>
       WOUT_GATES2 };    // wino_output_gates_kernel<2,4>
static_assert(WIN_TPI2 == DT_WIN_TPI2 && WIN_H2_4 == DT_WIN_H2_4 && WOUT_TPI6 == DT_WOUT_TPI6 && WOUT_GATES2 == DT_WOUT_GATES2,
              "the codes dt_wino_input / dt_wino_output report (mi355_dt.h)");
struct WinoLaunch { int form; unsigned grid, threads; };
WinoLaunch choose_wino_input(const WinoArgs &a);
WinoLaunch choose_wino_output(const WinoArgs &a, int gates);
// fused Winograd F(4x4,3x3) for the early layers (Cin 32 / 64 / 128 -> Cout 64 / 128 / 256: conv_2, conv_3, conv_5; conv_6 / conv_8 on request), wino4s_fused.hip
struct Wino4FusedArgs {
    const float *in;     // NHWC, pixel stride in_ld, frame stride in_bs
    long long in_bs;
    int in_ld;
    int B, H, W, Cin, N;
    const float *u;      // wino4s_fused_pack layout
    const float *bias;   // [N]
    float slope;
    float *out;          // full-resolution output (pixel stride out_ld, frame stride out_bs) or null
    long long out_bs;
    int out_ld;
    float *out2;         // 2x2 max-pooled output [B][H/2][W/2][out2_ld] or null (exactly one of out / out2)
    int out2_ld;
    int nby, nbx;        // set by the launcher
    const float *zeros;  // >= 16 B of device zeros: DMA source of out-of-image patch pixels (wino4s_fused.hip)
    unsigned *amax_out;  // wino4s_fused.hip: non-null = max |x| over the stored outputs into this slot (dt_amax_publish)
};
// U staged through LDS by DMA, in-register output transform, persistent over (block pair, 64-channel slice) items
int launch_wino4s_fused(hipStream_t st, const Wino4FusedArgs &a, const float *zeros);
void wino4s_fused_pack(const float *u36, int npad, int cin, int cout, float *dst);
// direct 3x3 convolution in the two-term fp16 form (conv3_h2.hip): conv_2 / conv_3 / conv_5's shapes
struct Conv3H2Args {
    const float *in;           // NHWC fp32, pixel stride in_ld, frame stride in_bs
    long long in_bs;
    int in_ld;
    int B, H, W, Cin, N, Np;   // Cin % 32 == 0; N % 64 == 0 output channels, Np rows in w / bias
    const unsigned short *w;   // two fp16 terms of the scaled packed weights [2][9 Cin / 16][Np][16], k = ((ci / 32) * 9 + tap) * 32 + ci % 32
    const float *pscale;       // [1]: 1 / the weights' power of two
    const unsigned *amax;      // max-|x| slot of the input tensor
    const float *bias;         // [Np]
    float slope;
    float *out;                // full-resolution output (pixel stride out_ld, frame stride out_bs) or null
    long long out_bs;
    int out_ld;
    float *out2;               // 2x2 max-pooled output [B][H/2][W/2][out2_ld] or null (exactly one of out / out2)
    int out2_ld;
    const float *zeros;        // >= 16 B of device zeros: where the loads of out-of-image patch pixels point
    unsigned *amax_out;        // non-null: max |x| of the stored outputs into this slot
    int tiles_x, tiles_y;      // set by the launcher
    // the 1x1 layer fused behind (N = 128, no pooling: conv_3 -> conv_4): non-null w1 = apply it to the tile before anything is stored; `out` then is ITS
    // output [..][N1] (out_ld / out_bs describe it), amax_out its maximum
    const unsigned short *w1;  // two fp16 terms of the scaled 1x1 weights [2][N / 16][Np1][16]
    const float *pscale1;      // [1]
    const float *bias1;        // [N1]
    int N1, Np1;               // N1 <= 64 output channels, Np1 rows in w1
    float slope1;
};
int launch_conv3_h2(hipStream_t st, const Conv3H2Args &a);
bool conv3_h2_usable(const Conv3H2Args &a);
double conv3_h2_flops(const Conv3H2Args &a);
// split-bf16 batched GEMM of the F(6x6,3x3) layers (wino_gemm_s3.hip): fp32 operands as three bf16 terms, six MFMAs per product
struct GemmS3Args {
    const unsigned short *a;   // V terms  [P][3][K/16][Mp][16]   (winograd.hip split input transform) -- the Winograd GEMMs; null for a 1x1 layer:
    const float *a_f32;        // ... whose A operand is the producing layer's fp32 activation as it lies, [Mt][a_ld] (P = 1), split into its terms by the
    int a_ld;                  //     kernel when a wave reads its fragment
    const unsigned short *b;   // U terms  [P][3][K/16][Np][16]   (wino_s3_pack_weights)
    float *c;                  // M'       [P] planes of [Mt][ldc], plane stride c_ps floats
    long long c_ps;
    int P, Mt, Mp, N, Np, K, ldc;
    // a 1x1 layer through this kernel: bias as one extra K stage -- ones = [256][16] FLOATS, rows (1, 0, .., 0),
    // bias_s3 = [3][Np][16] terms of (bias[n], 0, .., 0); both null for the Winograd GEMMs.  act: LeakyReLU(slope) in the epilogue
    const unsigned short *ones, *bias_s3;
    int act;
    float slope;
    int half;                  // 0: the launcher chooses between 256-row tiles (one workgroup per CU) and 128-row tiles (two per CU); 1 / -1: force
    // the fp16 form (round 6): nt = 2 -- a / b hold TWO fp16 terms (hi, lo) of SCALED operands, [P][2][K/16][rows][16], three products per multiply
    int nt;                    // 0 / 3: three bf16 terms; 2: two fp16 terms
    const float *pscale;       // nt = 2: [P] epilogue factor of position p = 1 / (U's scale[p] * the static part of V's scale[p])
    const unsigned *amax;      // nt = 2: the DT_AMAX_SUB-word max-|x| slot of the tensor V was made from (bits of a non-negative float): V carries
                               //         dt_h2_base(amax) (x the static per-position factor), the epilogue multiplies by dt_h2_base_inv(amax)
    const float *bias;         // nt = 2, 1x1 form: fp32 bias [N] or null, added in the epilogue (ones / bias_s3 stay null)
    unsigned *amax_out;        // 1x1 form: non-null = max |x| over the stored outputs into this slot (dt_amax_publish)
};
// ---- scaling of the fp16 form's operands (wino_gemm_s3.hip header) ----------------------------------------------------------------
// max |x| of a tensor is kept as the integer bits of a non-negative float in a slot of DT_AMAX_SUB words (producers spread their atomicMax
// over the sub-slots; a reader takes the maximum).  base = 2^(14 - floor(log2 amax)): amax * base is in [2^14, 2^15), a factor 2 below
// fp16's largest finite value 65504.  The exponent field is clamped to [27, 240] (amax = 0 -> base 2^114 on zeros; nothing overflows).
#define DT_AMAX_SUB 16
// The sub-words of a slot lie on DISTINCT 128-byte lines (DT_AMAX_LINE words apart): the first resident round of a producer finds the slot at zero and every one
// of its waves performs the atomicMax -- on one line those serialise at one L2 channel (~12 ns each: 25 us for the ~2,000 waves of a small launch; round 6 measured
// it as +0.36 ms per batch-8 forward over 13 output transforms), on sixteen lines they spread over sixteen channels
#define DT_AMAX_LINE 32
#define DT_AMAX_WORDS (DT_AMAX_SUB * DT_AMAX_LINE)      // words per slot
__host__ __device__ inline unsigned dt_h2_expfield(unsigned amax_bits)
{
    const unsigned e = (amax_bits >> 23) & 0xffu;
    return e < 27u ? 27u : (e > 240u ? 240u : e);
}
__host__ __device__ inline float dt_h2_from_field(unsigned f)
{
    const unsigned u = f << 23;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}
__host__ __device__ inline float dt_h2_base(unsigned amax_bits) { return dt_h2_from_field(268u - dt_h2_expfield(amax_bits)); }       // 2^(14 - e)
__host__ __device__ inline float dt_h2_base_inv(unsigned amax_bits) { return dt_h2_from_field(dt_h2_expfield(amax_bits) - 14u); }   // 2^(e - 14)
// static part of V's scale: the 1-D input transform's rows have absolute coefficient sums 12.5 / 7.5 / 15 (F(6,3)) and 10 / 6 (F(4,3));
// row i of Bt d B is scaled by the power of two that brings its sum below 1, so |V[p] * f[xi] * f[nu]| < max |d|
__host__ __device__ inline float dt_h2_rowfac(int ts, int i)
{
    if (ts == 6) return (i == 3 || i == 4) ? 0.125f : 0.0625f;
    if (ts == 4) return (i == 3 || i == 4) ? 0.125f : 0.0625f;
    return 1.0f;
}
#ifdef __HIPCC__
__device__ __forceinline__ unsigned dt_amax_read(const unsigned *slot)      // wave-uniform
{
    unsigned v = slot[(threadIdx.x & (DT_AMAX_SUB - 1)) * DT_AMAX_LINE];
#pragma unroll
    for (int o = DT_AMAX_SUB / 2; o; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o);
        v = w > v ? w : v;
    }
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
// A producer's contribution to the slot of the tensor it writes: every lane brings the largest |value| it STORED (fmaxf: NaNs are skipped, like
// in absmax_kernel -- the same set of numbers gives the same word whichever kernel took the maximum); the wave's maximum goes to one of the
// slot's sub-words, and only if it is larger than what is there already (a relaxed read first: most waves find nothing to add)
__device__ __forceinline__ void dt_amax_publish(unsigned *slot, float am)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
    if ((threadIdx.x & 63) == 0) {
        const unsigned b = __float_as_uint(am);
        unsigned *s = slot + ((blockIdx.x + (threadIdx.x >> 6)) & (DT_AMAX_SUB - 1)) * DT_AMAX_LINE;
        if (b > __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(s, b);
    }
}
#endif
// fp32 <-> fp16 bits on the host, round to nearest even, subnormals kept (what v_cvt_f16_f32 does under the default mode)
unsigned short h2_f16_rne(float x);
float h2_f16_f32(unsigned short h);
void wino_h2_split_host(float x_scaled, unsigned short t[2]);
// U [P][npad][K] fp32 (host) -> two fp16 terms [P][2][K/16][npad][16] of U[p] * uscale[p] (host)
void wino_h2_pack_weights(const float *u, int P, int npad, int K, const float *uscale, unsigned short *dst);
int launch_wino_gemm_s3(hipStream_t st, const GemmS3Args &a, int cus);
bool wino_gemm_s3_usable(int Mt, int K, int N);
bool wino_gemm_s3_half_chosen(const GemmS3Args &a, int cus);
double wino_gemm_s3_flops(const GemmS3Args &a);
void wino_s3_split_host(float x, unsigned short t[3]);
void wino_s3_pack_weights(const float *u, int P, int npad, int K, unsigned short *dst);
int launch_wino_input(hipStream_t st, const WinoArgs &a);
// U [P][npad][K] fp32 (device) -> split-bf16 [P][3][K/16][npad][16] (device)
int launch_wino_s3_pack(hipStream_t st, const float *u, int P, int npad, int K, unsigned short *dst);
int launch_wino_output(hipStream_t st, const WinoArgs &a, int gates);
bool wino_output_fills_amax(const WinoArgs &a, int gates);
// max |x| of `planes` tensors of rows x cols floats (row stride ld, plane stride plane_stride) -> slots[planes][DT_AMAX_SUB] (zeroed here)
int launch_absmax(hipStream_t st, const float *x, long long rows, int cols, long long ld, int planes, long long plane_stride, unsigned *slots, bool zero = true);
// U [P][npad][K] fp32 (device) -> two fp16 terms [P][2][K/16][npad][16] + epilogue factors pscale[P] (device); ts: Winograd tile (0: plain GEMM operand)
int launch_wino_h2_pack(hipStream_t st, const float *u, int P, int npad, int K, int ts, unsigned *slots, unsigned short *dst, float *pscale);
void wino_pack_weights(int ts, const float *hwio, int cin_src, int cout_src, const int *cin_map, int cin_dst, const int *n_map,
                       int npad, const float *scale, float *dst);

// ---------------------------------------------------------------------------
// other kernels
// ---------------------------------------------------------------------------
// What launch_conv1_direct does with a call (plan_conv1, conv1.hip): rc 0 = launches, 2 = refuses the arguments (odd or non-positive H / W, B outside
// 1..65535, a negative slope, an unknown dtype); which of the four kernel instances runs, the tiles a workgroup walks along x, the grid, and whether
// the instance fills `amax_out`.  The codes are mi355_dt.h's DT_C1_* (dt_conv1 reports them).
enum { C1_MFMA_F32 = 0, C1_S3_U8_FULL = 1, C1_S3_U8 = 2, C1_S3_F32 = 3 };
struct Conv1Plan {
    int rc, inst, tpw, grid_x, grid_y, grid_z, fills_amax;
};
Conv1Plan plan_conv1(const void *frames, int dtype, int B, int H, int W, float slope, bool split /*both three-term tables are passed*/,
                     int force_tpw /*test only: 0 = the launcher's rule*/);
int launch_conv1_direct(hipStream_t st, const void *frames, int dtype, int B, int H, int W,
                        const float *w_packed /*[27][32]*/, const float *bias /*[32]*/,
                        const float *lut /*[256] or null*/, float slope, float *out /*[B,H/2,W/2,32]*/,
                        const unsigned *w3 = nullptr /*[2][3][64][4]*/, const unsigned *w3u8 = nullptr /*weights / 255: both set -> conv1_s3_kernel*/,
                        unsigned *amax_out = nullptr /*conv1_s3_kernel: max |x| of the outputs into this slot*/,
                        int force_tpw = 0 /*test only (dt_conv1), 0 in production*/);
#define C1_W3_WORDS 1540      // 1536 table words + 16 bytes of zeros: where conv1_s3_kernel points the loads of out-of-image pixels
void conv1_split_tables(const float *w /*[27][32]*/, bool scale255, unsigned *w3 /*[1536 of C1_W3_WORDS]*/);

int launch_decode(hipStream_t st, const float *netout, long long frame_stride, int batch, int GH, int GW, int NB,
                  int NC, float obj_thr, float nms_thr, const float *anchors_dev, int cap, float *boxes,
                  int *counts, float *classes, float *post, const float *frame_thr /*[batch][2] (obj, nms) or null*/,
                  float *scratch /*batch x decode_scratch_floats() floats for grids above 1920 cells, else null*/);
size_t decode_scratch_floats(int GH, int GW, int NB);

int launch_bbox_iou(hipStream_t st, const float *pairs, int n, float *iou);

int launch_associate(hipStream_t st, const float *boxes, const int *counts, int n_clips, int T, int cap,
                     float thr, int *ids, int *nids);
// Association state of the stream slots (dt_associate_stream, dt_associate_stream_mem): clip i of the call continues slot slots[i].  Per slot its
// TRACK TABLE of up to tcap entries -- boxes [tcap][8] (x, y, w, h, -, label, -, -), ids [tcap], ages [tcap] -- and meta = STREAM_META ints
// (stream_state.hip).  The entries of age 0, the last frame the slot saw in decode order, lead the table; the aged entries follow them.
// dt_associate_stream reads and leaves the age-0 entries only (the rule with max_age = 0) and never touches `ages`.
struct AssocCarry {
    const int *slots;   // [n_clips] on the device; null = the stateless launch
    float *boxes;       // [n_slots][tcap][8]
    int *ids;           // [n_slots][tcap]
    int *ages;          // [n_slots][tcap]; read for the entries behind the age-0 ones only
    int *meta;          // [n_slots][STREAM_META]
    int tcap;           // entries per slot
    float *vel = nullptr;    // [n_slots][tcap][2] track velocities (vx, vy), dt_associate_stream_motion only; null in every other launch
    int *vstamp = nullptr;   // [n_slots] meta[SM_ASSOC_FRAMES] as the last motion call left it: the slot's velocities belong to its table only
                             // while the two agree (0 and a saturated counter: they never do, and every velocity reads as 0)
    int *hits = nullptr;     // [n_slots][tcap] frames in which each track had a box, dt_associate_stream_tracks only; null in every other launch
    int *hstamp = nullptr;   // [n_slots] as vstamp, for `hits`: written by the track read-out call alone, so after any other association entry
                             // the two differ and every entry reads as hits = 1
};
int launch_associate_stream(hipStream_t st, const float *boxes, const int *counts, int n_clips, int T, int cap,
                            float thr, int *ids, int *nids, const AssocCarry &carry);

// The track table (associate.hip:associate_table_kernel): one kernel at three LEVELS, each of which holds what the one below it
// holds and compiles none of what the ones above it add.
//   ASSOC_MEMORY  entries with ages: a lost track keeps its id for up to max_age frames (dt_associate_mem)
//   ASSOC_MOTION  + a velocity per entry, matched where it predicts the entry (dt_associate_motion); reads and writes vstamp
//   ASSOC_TRACKS  + a hit count per entry, the read-out of the confirmed entries and the match policies (dt_associate_tracks[_match]);
//                 reads and writes both stamps
// (ASSOC_FRAME, the previous-frame rule of associate_kernel, is a level of the host entries only: network.hip:associate_entry.)
enum { ASSOC_FRAME = 0, ASSOC_MEMORY = 1, ASSOC_MOTION = 2, ASSOC_TRACKS = 3 };
struct TrackReadout {   // ASSOC_TRACKS only; tracks / tinfo / tcounts: all three or none
    int *hits;          // [n_clips][T][cap] hits of each box's track after its frame, -1 in unused entries; may be null
    float *tracks;      // [n_clips][T][tcap][DT_TRACK_FLOATS]
    int *tinfo;         // [n_clips][T][tcap][DT_TRACK_INTS]
    int *tcounts;       // [n_clips][T]
};
// The scored two-pass match (dt_associate_tracks_scored; DESIGN.md "Track scores"): a box is HIGH when its float `at` is >= high.  Pass 1
// assigns the HIGH boxes as dt_associate_tracks_assign does, pass 2 the LOW boxes to the entries still unclaimed with age <= min(max_age,
// max_age_low) at thr_low (max_age_low = -1: no pass 2); an unclaimed box opens an id only with a score >= fresh and is dropped otherwise.
struct AssocScore {
    int at;             // 0..7: the float of a box that holds its score
    float high, fresh;
    float thr_low;
    int max_age_low;    // >= -1
};
struct AssocNoScore {}; // what the kernel's instances without ASSOC_MATCH_SCORED get in its place
struct AssocTableArgs {
    const float *boxes; // [n_clips][T][cap][DT_BOX_FLOATS]
    const int *counts;  // [n_clips][T]
    int T, cap;
    float thr;
    int max_age, tcap;
    float gain;         // from ASSOC_MOTION on
    int min_hits;       // ASSOC_TRACKS
    int *ids, *nids;    // [n_clips][T][cap], [n_clips]
    int *gaps;          // [n_clips][T][cap]; may be null
    TrackReadout out;
    AssocCarry carry;   // slots == null: the stateless launch
    // which instantiation the launcher picks; the kernel gets neither.  The launcher hands the members above to the kernel as its
    // parameters, one by one: a struct parameter is fetched from the argument segment in other blocks than scalar parameters are, and
    // at the tracks level (106 SGPRs, some kept in VGPR lanes) that changed where the spills fall.
    int level;         // ASSOC_MEMORY .. ASSOC_TRACKS
    int match;          // the track match policy, DT_MATCH_* bits (0 = decode order within a label); non-zero at ASSOC_TRACKS only
    bool assign;        // the optimal assignment (dt_associate_tracks_assign): ASSOC_TRACKS only, match 0 or DT_MATCH_ANY_LABEL
    bool scored;        // the two passes by detection score (dt_associate_tracks_scored): with `assign` only
    AssocScore score;   // read when `scored`
};
// The kernel's MATCH template value: the call's DT_MATCH_* bits and, for the assignment entries, ASSOC_MATCH_ASSIGN -- a bit of the
// launcher's own, never accepted from a public `match` argument (the match entries refuse 4 as they always did).
#define ASSOC_MATCH_ASSIGN 4
#define ASSOC_MATCH_SCORED 8      // the scored entries' two passes around the assignment: another launcher's bit, beside ASSOC_MATCH_ASSIGN only
inline int assoc_kernel_match(const AssocTableArgs &a) { return a.match | (a.assign ? ASSOC_MATCH_ASSIGN : 0) | (a.scored ? ASSOC_MATCH_SCORED : 0); }
#define ASSIGN_TILE_STRIDE 65     // words per row of the register form's weight tile: odd, so a column's 64 words fall in 64 banks
#define ASSIGN_INF 0x7fffffff     // assign_max_kernel's and the assignment match's "no reduced cost yet"
// dynamic LDS the launch needs: none in the register form (tcap <= 64, T <= 64) but the best-IoU-first order's keys [cap][64] or the
// assignment's weights [cap][65] and 128 words of pairs; in the general form two tables of 7 / 9 / 10 words per entry, the frame's
// gaps, three more words per box for the best-IoU-first order and the assignment, and the assignment's 6 * (tcap + 1) solver words; the
// scored passes add one word per box (its score) to the general form and nothing to the register form.
// match: the kernel's MATCH value (assoc_kernel_match)
size_t assoc_table_lds_bytes(int level, int T, int cap, int tcap, int match);
// 0: launched (or, n_clips <= 0, nothing to launch); 1: device error; 2: argument error, nothing launched -- T or cap < 1, tcap < cap or
// beyond the meta word's 16 bits, max_age < 0, a table beyond 160 KB of LDS, carry.tcap != tcap, a stream launch without the level's
// slot arrays; from ASSOC_MOTION on a gain outside [0, 1] or NaN; at ASSOC_TRACKS min_hits < 1, a partial read-out triple, match outside 0..3, assign below
// ASSOC_TRACKS or with DT_MATCH_BEST_FIRST, scored without assign or with score.at outside 0..7, a NaN score.high / fresh / thr_low, max_age_low < -1
int launch_associate_table(hipStream_t st, const AssocTableArgs &a, int n_clips);

__device__ __forceinline__ float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The reference's box IoU, shared by decode.hip (NMS), associate.hip and score.hip (track scoring): one definition, and these files are
// compiled with -ffp-contract=off -- numpy's float32 arithmetic rounds after every multiply and add, so no FMA may be formed here;
// the pragma in each body says so for any other file that comes to use them.
// utils.py:175-188
__device__ __forceinline__ float interval_overlap_ref(float x1, float x2, float x3, float x4)
{
#pragma clang fp contract(off)
    if (x3 < x1) {
        if (x4 < x1) return 0.0f;
        return fminf(x2, x4) - x1;
    } else {
        if (x2 < x3) return 0.0f;
        return fminf(x2, x4) - x3;
    }
}

// utils.py:155-173 (centre-format boxes)
__device__ __forceinline__ float bbox_iou_ref(float ax, float ay, float aw, float ah, float bx, float by, float bw,
                                              float bh)
{
#pragma clang fp contract(off)
    const float x1_min = ax - aw / 2, x1_max = ax + aw / 2;
    const float y1_min = ay - ah / 2, y1_max = ay + ah / 2;
    const float x2_min = bx - bw / 2, x2_max = bx + bw / 2;
    const float y2_min = by - bh / 2, y2_max = by + bh / 2;
    const float iw = interval_overlap_ref(x1_min, x1_max, x2_min, x2_max);
    const float ih = interval_overlap_ref(y1_min, y1_max, y2_min, y2_max);
    const float inter = iw * ih;
    const float a1 = aw * ah;
    const float a2 = bw * bh;
    const float uni = (a1 + a2) - inter;
    return inter / uni;
}

// maximum of an unsigned value over the 64 lanes (wave-uniform result): four DPP row shifts leave each row's maximum in
// its last lane (lanes shifted in from outside a row read 0), four lane reads and scalar max finish
__device__ __forceinline__ unsigned wave_umax_dpp(unsigned v)
{
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 15), b = (unsigned)__builtin_amdgcn_readlane((int)v, 31);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 47), d = (unsigned)__builtin_amdgcn_readlane((int)v, 63);
    return max(max(a, b), max(c, d));
}

// track scoring (score.hip:track_score_kernel): CLEAR-MOT counts of hypotheses against ground-truth tracks, one wavefront per clip.
// The object table, the frame's ground-truth rows and its hypotheses live in LDS: 8 * ocap + 11 * gcap + 7 * hcap words.
struct ScoreArgs {
    const float *gt_boxes;   // [n][T][gcap][DT_BOX_FLOATS]
    const int *gt_counts;    // [n][T]
    const int *gt_ids;       // [n][T][gcap]
    const float *hyp_boxes;  // [n][T][hcap][8]
    const int *hyp_counts;   // [n][T]
    const int *hyp_ids;      // [n][T][hcap][id_stride], the id in word 0
    int gcap, hcap, id_stride, label_at, T, ocap;
    float thr;
    int *totals;             // [n][DT_SCORE_INTS]
    int *objs;               // [n][ocap][DT_SCORE_OBJ_INTS]
    int *nobjs;              // [n]
    int *fcounts;            // [n][T][4] or null
    int *match;              // [n][T][gcap] or null
    float *miou;             // [n][T][gcap], null exactly when match is
};
size_t track_score_lds_bytes(int gcap, int hcap, int ocap);      // dynamic LDS the launch needs; dt_track_score refuses more than 160 KB
// 0: launched; 1: device error.  flags: DT_SCORE_* bits.  The arguments are dt_track_score's, validated there (n_clips > 0, the LDS fits).
int launch_track_score(hipStream_t st, const ScoreArgs &a, int n_clips, int flags);

// identity scoring (identity.hip, DESIGN.md "Identity scoring"): the overlap of ground-truth trajectories with hypothesis trajectories,
// one wavefront per clip, and an exact integer maximum-weight assignment, one wavefront per problem.  The inputs are ScoreArgs'.
struct IdentArgs {
    const float *gt_boxes;   // [n][T][gcap][DT_BOX_FLOATS]
    const int *gt_counts;    // [n][T]
    const int *gt_ids;       // [n][T][gcap]
    const float *hyp_boxes;  // [n][T][hcap][8]
    const int *hyp_counts;   // [n][T]
    const int *hyp_ids;      // [n][T][hcap][id_stride], the id in word 0
    int gcap, hcap, id_stride, label_at, T, acap, bcap;
    float thr;
    int *sizes;              // [n][DT_IDENT_INTS]
    int *gt_tab;             // [n][acap][2]
    int *hyp_tab;            // [n][bcap][2]
    int *overlap;            // [n][acap][bcap]
};
size_t identity_overlap_lds_bytes(int gcap, int hcap, int acap, int bcap);      // dt_identity_overlap refuses more than 160 KB
// 0: launched; 1: device error.  flags: DT_SCORE_* bits; without DT_SCORE_RESUME the overlap is zeroed on the stream first.
int launch_identity_overlap(hipStream_t st, const IdentArgs &a, int n_clips, int flags);
// (identity.hip and hota.hip) Rows [0, nr) of a frame, ids r_id: r_ent[r] becomes the table row of the id, opened if it is new and the table has room, else -1.
// t_id / t_n [cap] are the table (ids distinct), nt its rows in use.  Returns the boxes whose id found the table full (wave-uniform).
__device__ __forceinline__ int open_trajectories(volatile int *r_id, volatile int *r_ent, int nr, volatile int *t_id, volatile int *t_n,
                                                 int &nt, int cap, int lane)
{
    const int nt0 = nt;                                       // the table as the previous frame left it
    int over = 0;
    for (int r = lane; r < nr; r += 64) {
        const int id = r_id[r];
        int e = -1;
        if (id >= 0)
            for (int k = 0; k < nt0; ++k) e = t_id[k] == id ? k : e;
        r_ent[r] = e;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int r0 = 0; r0 < nr; r0 += 64) {
        const int r = r0 + lane;
        unsigned long long fresh = __ballot(r < nr && r_ent[r] < 0 && r_id[r] >= 0);
        while (fresh) {
            const int rr = r0 + __ffsll((long long)fresh) - 1;
            const int v = r_id[rr];
            int found = -1;                                   // a lower row of this frame may have opened the trajectory
            for (int k0 = nt0; k0 < nt; k0 += 64) {
                const int k = k0 + lane;
                const unsigned long long bal = __ballot(k < nt && t_id[k] == v);
                if (bal) {
                    found = k0 + __ffsll((long long)bal) - 1;
                    break;
                }
            }
            if (found < 0) {
                if (nt < cap) {
                    found = nt++;
                    if (lane == 0) { t_id[found] = v; t_n[found] = 0; }
                } else {
                    ++over;
                }
            }
            if (found >= 0 && lane == 0) r_ent[rr] = found;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            fresh &= fresh - 1ull;
        }
    }
    for (int r = lane; r < nr; r += 64) {
        const int e = r_ent[r];
        if (e >= 0) atomicAdd(const_cast<int *>(t_n + e), 1);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    return over;
}

struct AssignArgs {
    const int *w;            // [n][rcap][ccap]
    const int *dims;         // [n][stride], rows in word rows_at, columns in word cols_at
    int rcap, ccap, stride, rows_at, cols_at;
    int *row_to_col;         // [n][rcap]
    int *col_to_row;         // [n][ccap]
    long long *total;        // [n]
};
size_t assign_max_lds_bytes(int rcap, int ccap);                                // dt_assign_max refuses more than 160 KB
int launch_assign_max(hipStream_t st, const AssignArgs &a, int n);              // 0: launched; 1: device error

// HOTA scoring (hota.hip, DESIGN.md "HOTA scoring"): the alignment P of ground-truth with hypothesis trajectories over a clip (one
// wavefront per clip), the weights W of every frame's match from the finished P (one wavefront per frame; dt_assign_max solves them), and
// the counts per IoU level of the matched pairs (one wavefront per frame).  Integers only; the inputs are ScoreArgs'.
struct HotaArgs {
    const float *gt_boxes;   // [n][T][gcap][DT_BOX_FLOATS]
    const int *gt_counts;    // [n][T]
    const int *gt_ids;       // [n][T][gcap]
    const float *hyp_boxes;  // [n][T][hcap][8]
    const int *hyp_counts;   // [n][T]
    const int *hyp_ids;      // [n][T][hcap][id_stride], the id in word 0
    int gcap, hcap, id_stride, label_at, T, acap, bcap;
    int *sizes;              // [n][DT_IDENT_INTS]            written by the alignment, read by the weights
    int *gt_tab;             // [n][acap][2]                  likewise
    int *hyp_tab;            // [n][bcap][2]                  likewise
    long long *align;        // [n][acap][bcap]               likewise
    int *w;                  // [n][T][gcap][hcap]            the weights' outputs from here on; null for the alignment
    int *dims;               // [n][T][2]
    int *gt_ent;             // [n][T][gcap]
    int *hyp_ent;            // [n][T][hcap]
};
struct HotaCountArgs {
    const float *gt_boxes;   // [n][T][gcap][DT_BOX_FLOATS]
    const float *hyp_boxes;  // [n][T][hcap][8]
    const int *dims;         // [n][T][2]
    const int *gt_ent;       // [n][T][gcap]
    const int *hyp_ent;      // [n][T][hcap]
    const int *row_to_col;   // [n * T][gcap]
    int gcap, hcap, T, acap, bcap, n_thr;
    float thr[DT_HOTA_MAX_THR];
    int *tp;                 // [n][n_thr]
    long long *loc;          // [n][n_thr]
    int *pairs;              // [n][n_thr][acap][bcap]
};
size_t hota_align_lds_bytes(int gcap, int hcap, int acap, int bcap);            // dt_hota_align refuses more than 160 KB
size_t hota_weights_lds_bytes(int gcap, int hcap, int acap, int bcap);          // dt_hota_weights likewise
// 0: launched; 1: device error.  The arguments are validated by the entries (network.hip).  flags: DT_SCORE_* bits; without
// DT_SCORE_RESUME the alignment zeroes `align`, and the count zeroes tp, loc and pairs, on the stream first.
int launch_hota_align(hipStream_t st, const HotaArgs &a, int n_clips, int flags);
int launch_hota_weights(hipStream_t st, const HotaArgs &a, int n_clips, int flags);
int launch_hota_count(hipStream_t st, const HotaCountArgs &a, int n_clips, int flags);

// detection scoring (detscore.hip, DESIGN.md "Detection scoring"): the VOC match of detections against ground truth per frame, then the
// position of every detection in its class's score order over all frames.  Integers out; the ratios are taken on the host.
#define DT_DETSCORE_MAX_THR 16
struct DetMatchArgs {
    const float *det_boxes;  // [B][cap][DT_BOX_FLOATS]
    const int *det_counts;   // [B]
    const float *gt_boxes;   // [B][gcap][DT_BOX_FLOATS]
    const int *gt_counts;    // [B]
    const int *gt_flags;     // [B][gcap] or null (no row is ignored)
    int cap, gcap, score_at, B, NC, n_thr;
    float thr[DT_DETSCORE_MAX_THR];
    int *state;              // [n_thr][B][cap]
    int *best;               // [B][cap]
    float *iou;              // [B][cap]
};
struct DetRankArgs {
    const float *det_boxes;  // [B][cap][DT_BOX_FLOATS]
    const int *det_counts;   // [B]
    const int *state;        // [n_thr][B][cap]
    const float *gt_boxes;   // [B][gcap][DT_BOX_FLOATS]
    const int *gt_counts;    // [B]
    const int *gt_flags;     // [B][gcap] or null
    int cap, gcap, score_at, B, NC, n_thr;
    int *rank, *ctp;         // [n_thr][B][cap] each
    int *ngt;                // [NC]
    int *ndet, *ntp;         // [n_thr][NC] each
    // workspace of the call: offsets [B + 1] (rows in use before each frame; the last is their number N), then the rows in use in
    // flat-index order, one array per field: score, label (-1: outside 0..NC-1), the states of all thresholds two bits each, flat index
    int *offsets;
    float *c_score;
    int *c_label;
    unsigned *c_state;
    int *c_flat;
};
size_t detect_match_lds_bytes(int cap, int gcap);                // dynamic LDS of the match launch; dt_detect_match refuses more than 160 KB
size_t detect_rank_ws_bytes(int B, int cap);                     // the workspace above, in bytes
void detect_rank_ws_carve(DetRankArgs &a, void *ws);             // ... and its pointers
// 0: launched; 1: device error.  The arguments are those of dt_detect_match / dt_detect_rank, validated there (the LDS fits; B may be 0
// for the rank, which then only writes the totals)
int launch_detect_match(hipStream_t st, const DetMatchArgs &a);
int launch_detect_rank(hipStream_t st, const DetRankArgs &a);

// ---------------------------------------------------------------------------
// stream slots: state that outlives a call (stream_state.hip)
// ---------------------------------------------------------------------------
// meta row of a slot: entries in the stored track table, next free track id, frames the recurrence has seen (0 = the slot's h / c rows
// read as zeros whatever they hold), frames the association has seen.  A slot whose row is all zero is fresh (an empty table).
// SM_COUNT packs two counts, so that a reset stays one int4 store: bits 0..15 the age-0 entries (the last frame's boxes), bits 16..31 the
// aged entries behind them.
enum { SM_COUNT = 0, SM_NEXT_ID = 1, SM_FRAMES = 2, SM_ASSOC_FRAMES = 3, STREAM_META = 4 };
enum { SM_COUNT_MASK = 0xffff, SM_AGED_SHIFT = 16 };
// the call's slot list, from the caller's HOST array into the library-owned device list: the numbers travel as kernel arguments of a
// launch OUTSIDE any captured graph, so neither a host synchronisation nor pinned staging is needed.  reset_meta != null: the listed slots' meta rows are zeroed too
int launch_stream_slots(hipStream_t st, const int *h_slots, int n, int *d_list, int *reset_meta);
// vstamp[d_list[i]] = 0 for i < n: the listed slots' velocities are invalid (dt_stream_reset, after launch_stream_slots has filled d_list);
// the hit stamps (StreamTable::hstamp) are cleared by a second call
int launch_stream_clear_stamps(hipStream_t st, const int *d_list, int n, int *vstamp);
struct StateMove {
    const int *slots;      // [n] device
    float *tab_h, *tab_c;  // [n_slots][row]
    int *meta;             // [n_slots][STREAM_META]
    float *h, *c;          // the call's rows: stream i at h + i * h_bs / c + i * c_bs
    long long h_bs, c_bs;
    int n, row;            // row = G*G*U floats, a multiple of 32
    int scatter;           // 0: table -> call (gather);  1: call -> table, and the slots' frame counters advance by T
    int T;
};
int launch_stream_state_move(hipStream_t st, const StateMove &a);

int launch_heatmap_from_boxes(hipStream_t st, const float *box4, const double *xywh64, int n, int hs, float *out);
int launch_rect_from_heatmap(hipStream_t st, const float *heat, int n, int hs, float thresh, int *rect);
void ingest_tables(int src, int dst, int *tab);
int launch_ingest_resize(hipStream_t st, const unsigned char *src, int n, int Hs, int Ws, unsigned char *dst, int Hd,
                         int Wd, const int *xt, const int *yt);
// dt_ingest_frames: frames base .. base + count - 1 of a validated host descriptor array, as ONE launch whose arguments hold the descriptors
#define INGEST_FRAMES_PER_LAUNCH 64
int launch_ingest_frames(hipStream_t st, const dt_frame_desc *h_desc, int base, int count, unsigned char *dst, int Hd, int Wd);
// dt_ingest_views: views base .. base + count - 1 of a validated host array, as ONE launch whose arguments hold the views
#define INGEST_VIEWS_PER_LAUNCH 32
int launch_ingest_views(hipStream_t st, const dt_frame_view *h_views, int base, int count, unsigned char *dst, int Hd, int Wd);
// dt_boxes_map: frames base .. base + count - 1 of a validated host affine array [n][4], as ONE launch whose arguments hold the affines
#define BOXES_MAP_FRAMES_PER_LAUNCH 128
int launch_boxes_map(hipStream_t st, float *boxes, const int *counts, int base, int count, int cap, const float *h_affine);
#define DT_MAX_ANCHOR_BOXES 16
int launch_encode_targets(hipStream_t st, const int *objs, const int *counts, const int *dims, const double *aug,
                          int n, int cap, int GH, int GW, int NB, int C, int IH, int IW, int TBB,
                          const double *anchors_host, double *y, double *b);
int launch_top_box(hipStream_t st, const float *boxes, const int *counts, int n_frames, int cap, float *out4);

int launch_convlstm_gates_only(hipStream_t st, const float *xproj, long long xp_bs, int xp_ld, float *cstate,
                               long long c_bs, int c_ld, float *hout, long long h_bs, int h_ld, int B, int HW,
                               int U);

int launch_expand_rgb32(hipStream_t st, const void *frames, int dtype, long long n_pix, const float *lut, float *out);
int launch_unfold_bn(hipStream_t st, float *x, long long rows, int C, const float *scale, const float *shift);

int launch_global_maxpool(hipStream_t st, const float *in, int n, int HW, int C, float *out, int out_ld);
int launch_maxpool4_flatten(hipStream_t st, const float *in, int n, int H, int W, int C, float *out, int out_ld);
int launch_copy_cols(hipStream_t st, const float *src, int src_ld, float *dst, int dst_ld, long long rows,
                     int cols);
int launch_lstm_step(hipStream_t st, const float *xproj /*[B][4U] gate-interleaved*/, long long xp_bs,
                     const float *h_prev, long long h_bs, float *cstate, const float *Ur_packed /*[U][4U]*/,
                     float *h_out, long long ho_bs, int B, int U);
int launch_lstm_step0(hipStream_t st, const float *xproj, long long xp_bs, float *cstate, float *h_out,
                      long long ho_bs, int B, int U);
// The tiny trackers' stream slots (dt_tiny_stream_open; TinyStreamTable below): meta row of a slot = frames the slot has seen (0 = fresh:
// its h / c rows read as zeros whatever they hold), which of the two h copies is current, two spare words.  One row is one int4, like
// STREAM_META, so launch_stream_slots resets these rows too.
enum { TSM_FRAMES = 0, TSM_CUR = 1, TSM_META = 4 };
static_assert(TSM_META == STREAM_META, "launch_stream_slots zeroes one int4 per slot in either table");
struct LstmSlots {
    const int *list;     // [B] device: slot of track b of the call
    const int *meta;     // [n_slots][TSM_META]
    float *h;            // [2][n_slots][U]
    float *c;            // [n_slots][U]
    long long copy;      // floats from one h copy to the other: n_slots * U
    int first, last;     // the launch is the first / last step of its call (T = 1: both)
};
// launch_lstm_step with the state rows addressed per track through the slot list: c in the table row at every step, h_prev from the table
// on the first step (h_prev may be null there), h_t into the table's other copy on the last one
int launch_lstm_step_stream(hipStream_t st, const float *xproj, long long xp_bs, const float *h_prev, long long h_bs,
                            const float *Ur_packed, float *h_out, long long ho_bs, int B, int U, const LstmSlots &s);
// behind the last step: the listed slots' current copy flips and their frame counters advance by T
int launch_lstm_stream_advance(hipStream_t st, const int *list, int *meta, int B, int T);
int launch_dense_sigmoid(hipStream_t st, const float *h, long long h_bs, const float *Wd /*[U][O]*/,
                         const float *bd, int B, int U, int O, float *out, long long out_bs);

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct ProfEntry {
    int64_t launches = 0;
    double ms = 0, flops = 0, bytes = 0;
};

struct PendingEvent {
    hipEvent_t a, b;
    std::string name, tag;
};

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    long long layout = 0;      // ws_get_padded: the row layout whose pad columns are known to be zero (0: none yet)
};

// Owner of one device allocation: hipFree in the destructor and in reset(); move-only.  It does NOT synchronise: whoever releases memory that
// queued work may still read synchronises the stream first (network.hip: every loader does so once, before its first release).
template <class T> class DevMem {
    T *p = nullptr;

public:
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    DevMem(DevMem &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem &operator=(DevMem &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~DevMem() { reset(); }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(size_t n)   // n elements; what was held is released first
    {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T));
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    T *get() const { return p; }
    explicit operator bool() const { return p != nullptr; }
};
static_assert(!std::is_copy_constructible<DevMem<float>>::value && !std::is_copy_assignable<DevMem<float>>::value, "a device allocation has one owner");

// One Winograd-domain weight set in every device form it was built in (network.hip: upload_wino).  The 16-bit forms are the B operands of the split
// GEMM (wino_gemm_s3.hip); they are built from `u` on the device and live and die with it.
struct WinoWeights {
    int ts = 0;                   // output tile size 2 / 4 / 6; 0 = not built
    int cin = 0, npad = 0;
    DevMem<float> u;              // [P][npad][cin], P = (ts + 2)^2
    DevMem<unsigned short> s3;    // three bf16 terms [P][3][cin/16][npad][16], or empty
    DevMem<unsigned short> h2;    // two fp16 terms of U[p] * 2^su[p], [P][2][cin/16][npad][16], or empty
    DevMem<float> h2_pscale;      // with h2: the epilogue factors [P]
};

struct ConvLayer {
    int idx = 0, ks = 0, cin = 0, cout = 0, npad = 0;
    DevMem<float> wt;                 // packed
    DevMem<unsigned short> wt_s3;     // 1x1 layers: wt as split-bf16 terms [3][cin/16][npad][16] (wino_gemm_s3.hip) or empty
    DevMem<unsigned short> bias_s3;   // with wt_s3: the bias as the B rows of one extra K stage, [3][npad][16]
    DevMem<unsigned short> wt_h2;     // 1x1 layers: wt as two fp16 terms of the scaled weights [2][cin/16][npad][16] (wino_gemm_s3.hip's fp16 form) or empty
    DevMem<float> pscale_h2;          // with wt_h2: [1] the epilogue factor 1 / (the weights' power of two)
    DevMem<unsigned short> w3_h2;     // narrow 3x3 layers (conv_2 / 3 / 5's shapes): wt as two fp16 terms [2][9 cin / 16][npad][16] for conv3_h2.hip, or empty
    DevMem<float> pscale_w3;          // with w3_h2: [1]
    WinoWeights wino;                 // Winograd-domain weights (wide 3x3 layers) or not built
    WinoWeights wino_alt;             // F(4x4) weights kept next to F(6x6) ones for small-batch launches, or not built
    DevMem<float> fused4s;            // fused F(4x4,3x3) weights (wino4s_fused.hip: conv_2 / 3 / 5 / 6 / 8's shapes) or empty
    DevMem<float> bias;               // [npad]
    DevMem<float> scale;              // [cout]: folded BatchNorm scale (dt_detector_extract un-folds with it) or empty
    bool scale_has_zero = false;
};

// Tuning / test knobs.  ctx->pol is assigned by network.hip:policy_refresh only: in dt_create,
// dt_policy_reload, dt_policy_set and the two layer-level test entry points (dt_conv2d, dt_convlstm_step, so that the
// parity tests can force a policy on a live context through the environment).  No launch path calls getenv.
struct Policy {
    int wino = 1;            // DT_WINO: 0 never / 1 default policy / 2 everywhere the transforms are defined
    int wino_tile = 0;       // DT_WINO_TILE: 2/4/6 for every layer; 0 = default (6, recurrent convolution 4)
    int wino_mint = 0;       // DT_WINO_MINT: Winograd tiles from which a launch takes the transforms; 0 = the per-tile-size default (wino_runs)
    double wino_ws_gb = 96.0;   // DT_WINO_WS_GB: V + M' workspace above this -> direct form
    int mosaic = -1;         // DT_WINO_MOSAIC: 1 never, 2 .. 6 force, -1 = fewest tiles
    int fused4 = 1;          // DT_WINO_FUSED4: the fused F(4x4) kernel (wino4s_fused.hip): 0 never / 1 conv_2 / 3 / 5 (Cin <= 64) from 1024
                             //                 blocks / 3 also conv_6 / 8 (Cin 128) / 2 any eligible layer at any size.  Read at weight load (0) and per launch
    int trk_merge = 1;       // DT_TRK_MERGE: the ConvLSTM2D input projection reads conv_feat only -- conv_23 (1x1, linear: x_bbox = W23 feat + b23) is folded into the
                             //               projection's weights at load (W' = Wx[feat] + W23 Wx[bbox] in float64, b23 through a border-aware bias): K 1120 -> 1024 and no
                             //               conv_23 launch when the caller does not ask for the detector's grid; 0 = the two-step form.  Winograd path only (large batches)
    int pin = 0;             // DT_PIN: 1 = kernel selection independent of the batch a call happens to carry (the frame-sharded tracker runs the same
                             //         frame in batches of other sizes for other world sizes): Winograd wherever defined, no frame mosaics, the fused kernel
                             //         and the split GEMM at any size, one tile form, no split-K, no F(4x4)/F(6x6) choice by tile count.  Slower at small
                             //         batch; results -- and track ids -- then do not depend on the number of ranks (parallel.py: deterministic=True)
    int c3h2 = 1;            // DT_C3H2: conv_2 / conv_3 / conv_5 as DIRECT 3x3 convolutions in the two-term fp16 form (conv3_h2.hip) from 1024 16x16-pixel blocks
                             //          (where the fused F(4x4) fp32 kernel ran until round 5); 0 = the fused kernel; 2 = at any size (parity tests).  Needs the fp16
                             //          form (DT_S3_H2, not DT_PIN).  Read at weight load (0: no fp16 copy of the weights) and per launch
    int conv_cfg = -1;       // DT_CONV_CFG
    int s3_conv1 = 1;        // DT_S3_CONV1: conv_1 on the bf16 pipe with split operands (conv1_s3_kernel); 0 = conv1_mfma_kernel (fp32 MFMA)
    int s3 = 1;              // DT_S3: the F(6x6) layers' batched GEMMs on the bf16 matrix pipe with 3-term split operands (wino_gemm_s3.hip):
                             //        0 never (fp32 MFMA) / 1 where it wins (K >= 128, GEMM rows >= s3_minrows) / 2 wherever the shape allows
    int s3_minrows = 2048;   // DT_S3_MINROWS
    int s3_minrows_h2 = 64;  // ... the row threshold where the launch would take the fp16 form (three products per multiply: the split GEMM beats the fp32 MFMA
                             //     kernel from far fewer rows than the bf16 form does -- detector forward at 32 / 64 / 128 / 192 frames: 3.50 -> 2.85, 6.60 -> 4.45,
                             //     9.91 -> 7.17, 14.5 -> 10.2 ms; 64 rather than 128 for the 75 / 98 rows of the 13 x 13 layers at 12 / 16 frames; profiles/r06_experiments.txt section 10).
                             //     DT_S3_MINROWS, when set, is the threshold of BOTH forms
    int s3_h2 = 1;           // DT_S3_H2: the split GEMMs in the fp16 form -- two terms of SCALED operands, three products on v_mfma_f32_32x32x16_f16 (half the
                             //           matrix-pipe work and 4 instead of 6 bytes per operand element; wino_gemm_s3.hip) -- wherever the bf16 form would run; 0 = three
                             //           bf16 terms / six products (round 3).  Read at weight load (the fp16 terms are built then) and per launch.  DT_PIN takes the
                             //           bf16 form: the fp16 form's scale is the batch's max |x|, so its rounding of small elements depends on the batch
    int c3fuse = 1;          // DT_C3FUSE: conv_4 (1x1, 128 -> 64) applied inside conv_3's direct kernel (conv3_h2.hip, FUSE): one launch, no 128-channel tensor; 0 = two launches
    int h2_minframes = 12;   // DT_H2_MINFRAMES: a forward of fewer frames takes round 5's forms (bf16 terms, fused fp32 kernel) and its producers publish no max |x|:
                             //                  at batch 8 the publications (a dependent load + atomic at the tail of 40-us kernels) and the one stand-alone absmax pass
                             //                  cost 0.16 ms of a 1.26 ms forward and the fp16 form has nothing to win there (weights-bound GEMMs on the fp32 kernel).
                             //                  Detector forward with the fp16 form from 8 frames against from 32: batch 8 1.41 vs 1.26 ms, 12: 1.98 vs 1.81, 16: 2.13 vs 2.10,
                             //                  24: 2.29 vs 2.81 -- the crossover lay between 16 and 24 frames while every small producer paid ~25 us for its publication.
                             //                  With the sub-words of a slot on distinct cache lines (DT_AMAX_LINE) and the cooperative output transform publishing too
                             //                  (no stand-alone absmax passes): batch 8 1.25-1.31 vs 1.26, 12: 1.50 vs 1.81, 16: 1.74 vs 2.09, 20: 2.40 vs 2.53, 24: 1.91 vs 2.80
                             //                  (row threshold 64-96) -- from 12 frames
    int s3_half = 0;          // DT_S3_HALF: 128-row tiles / two workgroups per CU in the split GEMM: 0 where it needs fewer rounds (default) / 1 always (N % 256 == 0) / -1 never
    int s3_rec_minrows = 512; // DT_S3_REC_MINROWS: the ConvLSTM recurrent step's F(4x4) GEMM (gate update in its output transform) takes the split
                              //                    kernel from this many GEMM rows (48 clips at 13x13: 588); 0 = never
    int s3_rec_minrows_h2 = 16; // ... where the step would take the fp16 form (one clip at 13x13 = 16 rows: 5.30 -> 4.71 ms per 30-frame clip; 8 / 12 / 24 / 36 clips =
                                //     98 / 147 / 294 / 441 rows: 6-9 % of the whole tracking step); DT_S3_REC_MINROWS, when set, is the threshold of both forms
    int s3_1x1_mink = 256;   // DT_S3_1X1_MINK: ... only for 1x1 layers with at least this many input channels (conv_7 / 10 / 12 / 15 / 17 / 23; 512 while the
                             //                  producer had to write split rows -- the kernel reads the fp32 activation itself since round 4; conv_4 at
                             //                  K = 128, N = 64 measured 3.55 ms there against 2.85 on the fp32 kernel)
    int s3_1x1_minrows = 16384;   // DT_S3_1X1_MINROWS: ... and at least this many pixels: one split GEMM of a 1x1 layer has M / 256 row tiles and no split-K, so at
                                  // batch 8 (conv_10 / 12: 5408 rows = 22 workgroups) the fp32 kernel with split-K is faster (0.035 vs 0.061 ms)
    int s3_1x1 = 1;          // DT_S3_1X1: the 1x1 layers with N % 128 == 0 run on wino_gemm_s3.hip straight from the fp32 activation (the kernel splits
                             //            its A fragments itself); 0 = fp32 MFMA
    int amax_measure = 0;    // DT_AMAX_MEASURE: 1 = every fp16-form consumer measures its input's max |x| into its own slot (32 + i / 56 / 57) and ignores
                             //                  the producers' tags (the producers still publish): tests compare the published words with the measured ones
};

// The stream slots of a context (dt_stream_open): everything a stream carries from one call to the next, in device memory
struct StreamTable {
    int n_slots = 0, cap = 0;
    int tcap = 0;              // entries of a slot's track table (dt_stream_open: cap)
    int row = 0;               // floats per h / c row: G*G*U of the tracker the table was opened under
    DevMem<float> h, c;        // ConvLSTM state [n_slots][G*G][U]
    DevMem<float> boxes;       // the track table's boxes [n_slots][tcap][8]: the last frame's first, aged entries behind them
    DevMem<int> ids;           // ... their ids [n_slots][tcap]
    DevMem<int> ages;          // ... and ages [n_slots][tcap]
    DevMem<float> vel;         // ... and velocities [n_slots][tcap][2], written and read by dt_associate_stream_motion only
    DevMem<int> vstamp;        // [n_slots]: meta[SM_ASSOC_FRAMES] as the last motion call left it (AssocCarry::vstamp); 0 = no valid velocities
    DevMem<int> hits;          // ... and hit counts [n_slots][tcap], written and read by dt_associate_stream_tracks only
    DevMem<int> hstamp;        // [n_slots]: as vstamp, for the hit counts (AssocCarry::hstamp); 0 = no valid hit counts
    DevMem<int> meta;          // [n_slots][STREAM_META]
    DevMem<int> list;          // [n_slots]: the slot list of the running call, filled before its launches (never a kernel argument of a captured launch)
    std::vector<char> warm;    // host mirror of meta[SM_FRAMES] != 0: decides between the gates-only launch and a full step at t = 0
};

// The stream slots of the tiny trackers (dt_tiny_stream_open): the per-object LSTM's state, carried from one call to the next.  Apart from
// `streams`: a context may hold both tables, and no entry of one touches the other.
struct TinyStreamTable {
    int n_slots = 0;
    int U = 0;                 // units of the model the table was opened under
    DevMem<float> h;           // [2][n_slots][U]: two copies, used alternately -- a call reads meta[TSM_CUR] and writes the other (recurrent.hip)
    DevMem<float> c;           // [n_slots][U]
    DevMem<int> meta;          // [n_slots][TSM_META]
    DevMem<int> list;          // [n_slots]: the slot list of the running call (never a kernel argument of a captured launch)
};

struct dt_ctx {
    std::string err;
    Policy pol;
    int pin_override = -1;   // dt_policy_set("pin"): 0 / 1 instead of DT_PIN, -1 = follow DT_PIN
    hipStream_t stream = nullptr;
    // detector
    int image_h = 0, image_w = 0, cb = 0;   // cb = nb_box * (5 + nb_class): channels of conv_23
    float dec_anchors_host[64];   // last anchors handed to dt_decode (persistent staging of the caller's host array)
    int dec_anchors_n = 0;
    bool det_loaded = false;
    ConvLayer layers[24];   // 1..23
    DevMem<float> s3_ones;   // [256][16]: the A rows (1, 0, .., 0) that carry a 1x1 layer's bias through wino_gemm_s3.hip
    // max-|x| slots of the fp16 form (DT_AMAX_SUB words each; dt_internal.h: dt_h2_base).  Slot 0 holds 1.0 (|h_t| < 1: the ConvLSTM recurrent step);
    // slot i in 1..23: the OUTPUT of conv_i, filled by the epilogue of the kernel that writes it (network.hip: amax_begin zeroes them per forward);
    // 32 + i: the INPUT of conv_i where no producer measured it (absmax_kernel); 56: the tracker's z / conv_feat; 57, 58: test entry points;
    // 64..127: scratch of the weight packs
    DevMem<unsigned> amax;
    struct AmaxTag { const float *lo, *hi; int cols, slot; };   // the tensor that occupies [lo, hi), `cols` channels per pixel -> the slot that holds its max |x|
    bool h2_small = false;                   // the running call carries fewer than Policy::h2_minframes frames: no fp16 form, no max-|x| publication (call_begin)
    std::vector<AmaxTag> amax_tag;           // valid inside one API call only (call_begin), and until a layer writes into [lo, hi) (amax_forget)
    DevMem<float> conv1_w, conv1_b, lut255;
    DevMem<unsigned> conv1_w3, conv1_w3u8;   // split-bf16 weight tables of conv1_s3_kernel: w and w / 255 (conv1.hip:conv1_split_tables)
    std::vector<float> conv1_hwio32, conv1_scale, conv1_shift;   // host copy of conv_1 as a Cin = 32 layer (dt_detector_extract)
    // tracker head
    bool trk_loaded = false;
    int trk_units = 0, trk_cx = 0 /*padded z channels*/;
    DevMem<float> trk_wx, trk_bx;                 // input conv, N gate-interleaved
    DevMem<float> trk_wh;                         // recurrent conv
    WinoWeights trk_wx_wino, trk_wh_wino;         // their Winograd-domain forms, or not built
    WinoWeights trk_wxm_wino;                     // F(6x6) weights of the MERGED input projection (conv_23 folded in; 1024 input channels) or not built
    DevMem<float> trk_bx16;                       // its bias: [17][4U] gate-interleaved -- row 0 the interior bias, rows 1 + k the correction of border case k
    std::vector<float> conv23_hwio, conv23_bias;  // host copies of conv_23 ([1024][cb], [cb]) and of the ConvLSTM input kernel / bias (Keras HWIO, x_bbox first):
    std::vector<float> trk_hkernel, trk_hbias;    // what the merge is computed from, whichever of the two loaders runs second
    ConvLayer trk_out;                            // tconv_2 1x1 (idx 102): wt and bias only, so that it stays on the fp32 MFMA kernel
    // tiny tracker
    bool tiny_loaded = false;
    int tiny_D = 0, tiny_Dpad = 0, tiny_U = 0, tiny_O = 0, tiny_Opad = 0;
    DevMem<float> tiny_wx, tiny_bx, tiny_ur, tiny_wd, tiny_bd;
    StreamTable streams;
    TinyStreamTable tiny_streams;
    // workspaces (grown on demand)
    std::map<std::string, DevBuf> ws;
    int last_batch = 0;
    bool tap_feat = false, tap_netout = false;   // last forward wrote the library-owned 'feat' / 'netout' workspaces
    int ing_key[4] = {0, 0, 0, 0};   // (Hs, Ws, Hd, Wd) of the cached ingest tables
    // hipGraph replay of the launch-bound inner sequences (dt_graph_enable; network.hip:graphed)
    bool graph_on = false, capturing = false;
    hipStream_t gstream = nullptr;
    std::map<std::string, hipGraphExec_t> graphs;
    std::map<std::string, int> graph_seen;
    std::map<std::string, std::vector<AmaxTag>> graph_tags;   // amax_tag as a graphed sequence left it (re-applied on replay)
    int64_t graph_replays = 0, graph_captures = 0;
    // profiling
    bool prof = false;
    std::map<std::string, ProfEntry> prof_tab;
    std::vector<PendingEvent> pending;
};

int dt_fail(dt_ctx *ctx, int code, const char *fmt, ...);
float *ws_get(dt_ctx *ctx, const char *name, size_t bytes, bool zero_on_grow = false);
// rows of `width` floats of which only the first `used` are ever written: the pad columns [used, width) read zero
float *ws_get_padded(dt_ctx *ctx, const char *name, size_t bytes, int width, int used);

#define HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return dt_fail(ctx, DT_ERR_DEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                           __FILE__, __LINE__);                                                  \
    } while (0)

// profiling scope helper
struct ProfScope {
    dt_ctx *ctx;
    PendingEvent ev;
    bool on;
    ProfScope(dt_ctx *c, const char *name, double flops, double bytes, const char *tag = nullptr);
    ~ProfScope();
};
