// ingest.hip -- frame ingest: the  cv2.resize(image, (IMAGE_H, IMAGE_W))  step in front of
// the detector (models_detection/KerasYOLO.py:525-528, MultiObjDetTracker.py:301-304),
// on decoded uint8 HWC frames already in HBM.  The /255. that follows it in the reference is
// fused into conv_1, so the kernel's output is the uint8 network input.
//
// Definition (parity vs OpenCV itself is unpinned: cv2 is absent): OpenCV's
// 8-bit INTER_LINEAR scheme -- half-pixel centres, no anti-aliasing, 11-bit coefficients,
// ((b0*(S0>>4))>>16 + (b1*(S1>>4))>>16 + 2) >> 2 -- restated in oracle.c:orc_resize_bilinear_u8.
// Integer arithmetic only; the coefficient tables are built on the host with the oracle's
// formula, so the kernel is bit-exact against it.  (dt_ingest_frames' kernel further down -- NV12 / pitched frames at per-frame
// sizes -- computes the same coefficients on the device, operation for operation, and needs no table.)
//
// HBM-bound: one thread per output pixel (3 channels), 4 source pixels read, 3 bytes written;
// a wavefront writes 192 contiguous bytes.  Algorithmic bytes per frame: Hs*Ws*3 read (each
// source pixel is touched ~(Hd*Wd*4)/(Hs*Ws) times through L1/L2) + Hd*Wd*3 written.
#include <cmath>

#include "dt_internal.h"

struct IngestArgs {
    const unsigned char *src;
    unsigned char *dst;
    int n, Hs, Ws, Hd, Wd;
    const int *xt;   // [4][Wd]: x0, x1, a0, a1
    const int *yt;   // [4][Hd]: y0, y1, b0, b1
};

__global__ __launch_bounds__(256) void ingest_resize_kernel(IngestArgs p)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const long long f = blockIdx.z;
    if (x >= p.Wd) return;
    const int x0 = p.xt[x] * 3, x1 = p.xt[p.Wd + x] * 3, a0 = p.xt[2 * p.Wd + x], a1 = p.xt[3 * p.Wd + x];
    const int y0 = p.yt[y], y1 = p.yt[p.Hd + y], b0 = p.yt[2 * p.Hd + y], b1 = p.yt[3 * p.Hd + y];
    const unsigned char *s = p.src + f * p.Hs * p.Ws * 3;
    const unsigned char *r0 = s + (long long)y0 * p.Ws * 3, *r1 = s + (long long)y1 * p.Ws * 3;
    unsigned char *o = p.dst + ((f * p.Hd + y) * p.Wd + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int S0 = r0[x0 + c] * a0 + r0[x1 + c] * a1;
        const int S1 = r1[x0 + c] * a0 + r1[x1 + c] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        o[c] = (unsigned char)min(max(v, 0), 255);
    }
}

// ---------------------------------------------------------------------------
// dt_ingest_frames: NV12 / RGB24 frames at per-frame sizes and row pitches, one launch per 64 frames
// ---------------------------------------------------------------------------
// The descriptors of a launch travel as kernel arguments (64 x 40 bytes), the way stream_state.hip passes slot numbers: no
// upload, no workspace, nothing kept in the context.  blockIdx.z picks the frame, so everything read from the descriptor
// -- size, pitches, format -- is the same in every lane of a wave.
struct IngestFrameChunk { dt_frame_desc f[INGEST_FRAMES_PER_LAUNCH]; };
static_assert(sizeof(dt_frame_desc) == 40, "dt_frame_desc is 40 bytes: 64 of them are one launch's arguments");

// ingest_tables' row for destination index d, computed in place of a table look-up: the same operations in the same order, every one
// rounded on its own (an FMA for the product and the subtraction changes f in the last bit for some (src, dst, d))
__device__ __forceinline__ void ingest_coef(int src, int dst, int d, int &s0, int &s1, int &c0, int &c1)
{
#pragma clang fp contract(off)
    const double scale = (double)src / (double)dst;
    const double prod = ((double)d + 0.5) * scale;
    float f = (float)(prod - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= src - 1) { f = 0.0f; s = src - 1; }
    s0 = s;
    s1 = s + 1 < src ? s + 1 : src - 1;
    c0 = __float2int_rn((1.0f - f) * 2048.0f);
    c1 = __float2int_rn(f * 2048.0f);
}

// BT.601 limited range, the 20-bit fixed-point constants of OpenCV's 8-bit YUV420 conversions; (Y, U, V) in, (R, G, B) out, in place
__device__ __forceinline__ void nv12_to_rgb(int &c0, int &c1, int &c2)
{
    const int y = max(c0 - 16, 0) * 1220542, u = c1 - 128, v = c2 - 128;
    c0 = min(max((y + 1673527 * v + 524288) >> 20, 0), 255);
    c1 = min(max((y - 852492 * v - 409993 * u + 524288) >> 20, 0), 255);
    c2 = min(max((y + 2116026 * u + 524288) >> 20, 0), 255);
}

__global__ __launch_bounds__(256) void ingest_frames_kernel(IngestFrameChunk c, unsigned char *dst, int Hd, int Wd)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= Wd) return;
    const dt_frame_desc &d = c.f[blockIdx.z];
    const int Hs = d.height, Ws = d.width;
    const bool nv12 = (d.format & ~DT_PIX_SWAP_RB) == DT_PIX_NV12, swap = (d.format & DT_PIX_SWAP_RB) != 0;
    int xs[2], ys[2], a[2], b[2];
    ingest_coef(Ws, Wd, x, xs[0], xs[1], a[0], a[1]);
    ingest_coef(Hs, Hd, y, ys[0], ys[1], b[0], b[1]);      // (the same in every lane: y is blockIdx.y)
    const unsigned char *p0 = static_cast<const unsigned char *>(d.d_plane0);
    // RGB24 keeps its three bytes side by side in plane 0; NV12 has Y in plane 0 and the (U, V) pair of the 2x2 block in plane 1.  Only the
    // ADDRESSES depend on the format, through selects on wave-uniform values: the byte loads below are the same instructions for both and
    // all of them are issued before the first wait (a load under a condition makes hipcc wait for each one on its own)
    const unsigned char *pc = nv12 ? static_cast<const unsigned char *>(d.d_plane1) : p0 + 1;
    const long long pitch_c = nv12 ? d.pitch1 : d.pitch0;
    const int sh = nv12 ? 1 : 0;                           // chroma is shared by 2x2 pixels
    const int m0 = nv12 ? 1 : 3, mc = nv12 ? 2 : 3;        // bytes from one pixel (pair) of a row to the next
    int px[2][2][3];      // [row][column][channel]
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned char *row0 = p0 + (long long)ys[r] * d.pitch0;
        const unsigned char *rowc = pc + (long long)(ys[r] >> sh) * pitch_c;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int o0 = xs[k] * m0, oc = (xs[k] >> sh) * mc;
            px[r][k][0] = row0[o0];
            px[r][k][1] = rowc[oc];
            px[r][k][2] = rowc[oc + 1];
        }
    }
    if (nv12) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 2; ++k) nv12_to_rgb(px[r][k][0], px[r][k][1], px[r][k][2]);
    }
    unsigned char *o = dst + (((long long)blockIdx.z * Hd + y) * Wd + x) * 3;
    int out[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int S0 = px[0][0][ch] * a[0] + px[0][1][ch] * a[1];
        const int S1 = px[1][0][ch] * a[0] + px[1][1][ch] * a[1];
        const int v = (((b[0] * (S0 >> 4)) >> 16) + ((b[1] * (S1 >> 4)) >> 16) + 2) >> 2;
        out[ch] = min(max(v, 0), 255);
    }
    // the blend works on each channel alone, so exchanging channels 0 and 2 of the result is exchanging them in the converted pixels
    o[0] = (unsigned char)(swap ? out[2] : out[0]);
    o[1] = (unsigned char)out[1];
    o[2] = (unsigned char)(swap ? out[0] : out[2]);
}

// h_desc: a validated host array; frame i of dst [n][Hd][Wd][3] comes from h_desc[i]
int launch_ingest_frames(hipStream_t st, const dt_frame_desc *h_desc, int base, int count, unsigned char *dst, int Hd, int Wd)
{
    if (count <= 0) return 0;
    if (count > INGEST_FRAMES_PER_LAUNCH || Hd <= 0 || Hd > 65535 || Wd <= 0) return 2;
    IngestFrameChunk c;
    for (int j = 0; j < INGEST_FRAMES_PER_LAUNCH; ++j) c.f[j] = h_desc[base + (j < count ? j : 0)];
    dim3 grid((unsigned)((Wd + 255) / 256), (unsigned)Hd, (unsigned)count);
    hipLaunchKernelGGL(ingest_frames_kernel, grid, dim3(256), 0, st, c, dst + (size_t)base * Hd * Wd * 3, Hd, Wd);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------
// dt_ingest_views: a crop of each frame, resized into a rectangle of the output, a fill colour around it; one launch per 32 views
// ---------------------------------------------------------------------------
// ingest_frames_kernel with a source rectangle and a destination rectangle.  What that kernel learned is kept: only
// ADDRESSES are selected, every load is issued before the first wait, no load sits under a lane-divergent condition.  A lane outside
// the destination rectangle clamps its column into it -- it loads what the nearest column inside loads -- and selects the fill at the
// store.  blockIdx.y and the view are the same in every lane, so an output row that lies wholly in the fill leaves through a
// wave-uniform branch before any coefficient or load.
struct IngestViewChunk { dt_frame_view v[INGEST_VIEWS_PER_LAUNCH]; };
static_assert(sizeof(dt_frame_view) == 80, "dt_frame_view is 80 bytes");
static_assert(sizeof(IngestViewChunk) + sizeof(unsigned char *) + 2 * sizeof(int) <= 4096, "a launch's views and its other arguments fit HIP's 4096 bytes of kernel arguments");

__global__ __launch_bounds__(256) void ingest_views_kernel(IngestViewChunk c, unsigned char *dst, int Hd, int Wd)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= Wd) return;
    const dt_frame_view &v = c.v[blockIdx.z];
    unsigned char *o = dst + (((long long)blockIdx.z * Hd + y) * Wd + x) * 3;
    // the fill's three bytes and reserved0 (0) as one word of the arguments, read once for both ways out
    const unsigned fw = (unsigned)v.fill[0] | (unsigned)v.fill[1] << 8 | (unsigned)v.fill[2] << 16;
    const int f0 = fw & 255, f1 = (fw >> 8) & 255, f2 = fw >> 16;
    const int ry = y - v.dst_y;
    if (ry < 0 || ry >= v.dst_h) {                         // (the same in every lane) a row of fill: nothing is read
        o[0] = (unsigned char)f0;
        o[1] = (unsigned char)f1;
        o[2] = (unsigned char)f2;
        return;
    }
    const dt_frame_desc &d = v.frame;
    const bool nv12 = (d.format & ~DT_PIX_SWAP_RB) == DT_PIX_NV12, swap = (d.format & DT_PIX_SWAP_RB) != 0;
    const int rx = x - v.dst_x;
    const bool inside = rx >= 0 && rx < v.dst_w;
    int xs[2], ys[2], a[2], b[2];
    ingest_coef(v.src_w, v.dst_w, min(max(rx, 0), v.dst_w - 1), xs[0], xs[1], a[0], a[1]);
    ingest_coef(v.src_h, v.dst_h, ry, ys[0], ys[1], b[0], b[1]);      // (the same in every lane)
    // from here on the indices are those of the frame: chroma is addressed by the absolute position, so a crop may start at an odd pixel
    xs[0] += v.src_x; xs[1] += v.src_x;
    ys[0] += v.src_y; ys[1] += v.src_y;
    const unsigned char *p0 = static_cast<const unsigned char *>(d.d_plane0);
    const unsigned char *pc = nv12 ? static_cast<const unsigned char *>(d.d_plane1) : p0 + 1;
    const long long pitch_c = nv12 ? d.pitch1 : d.pitch0;
    const int sh = nv12 ? 1 : 0;
    const int m0 = nv12 ? 1 : 3, mc = nv12 ? 2 : 3;
    int px[2][2][3];      // [row][column][channel]
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned char *row0 = p0 + (long long)ys[r] * d.pitch0;
        const unsigned char *rowc = pc + (long long)(ys[r] >> sh) * pitch_c;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int o0 = xs[k] * m0, oc = (xs[k] >> sh) * mc;
            px[r][k][0] = row0[o0];
            px[r][k][1] = rowc[oc];
            px[r][k][2] = rowc[oc + 1];
        }
    }
    if (nv12) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 2; ++k) nv12_to_rgb(px[r][k][0], px[r][k][1], px[r][k][2]);
    }
    int out[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int S0 = px[0][0][ch] * a[0] + px[0][1][ch] * a[1];
        const int S1 = px[1][0][ch] * a[0] + px[1][1][ch] * a[1];
        const int t = (((b[0] * (S0 >> 4)) >> 16) + ((b[1] * (S1 >> 4)) >> 16) + 2) >> 2;
        out[ch] = min(max(t, 0), 255);
    }
    // the fill is written as it is: the channel exchange is the frame's, not the fill's
    o[0] = (unsigned char)(inside ? (swap ? out[2] : out[0]) : f0);
    o[1] = (unsigned char)(inside ? out[1] : f1);
    o[2] = (unsigned char)(inside ? (swap ? out[0] : out[2]) : f2);
}

// h_views: a validated host array; frame i of dst [n][Hd][Wd][3] comes from h_views[i]
int launch_ingest_views(hipStream_t st, const dt_frame_view *h_views, int base, int count, unsigned char *dst, int Hd, int Wd)
{
    if (count <= 0) return 0;
    if (count > INGEST_VIEWS_PER_LAUNCH || Hd <= 0 || Hd > 65535 || Wd <= 0) return 2;
    IngestViewChunk c;
    for (int j = 0; j < INGEST_VIEWS_PER_LAUNCH; ++j) c.v[j] = h_views[base + (j < count ? j : 0)];
    dim3 grid((unsigned)((Wd + 255) / 256), (unsigned)Hd, (unsigned)count);
    hipLaunchKernelGGL(ingest_views_kernel, grid, dim3(256), 0, st, c, dst + (size_t)base * Hd * Wd * 3, Hd, Wd);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// same formula as oracle.c:orc_resize_tables
void ingest_tables(int src, int dst, int *tab /*[4][dst]*/)
{
    const double scale = (double)src / (double)dst;
    for (int d = 0; d < dst; ++d) {
        float f = (float)(((double)d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (s < 0) { f = 0.0f; s = 0; }
        if (s >= src - 1) { f = 0.0f; s = src - 1; }
        tab[d] = s;
        tab[dst + d] = s + 1 < src ? s + 1 : src - 1;
        tab[2 * dst + d] = (int)lrintf((1.0f - f) * 2048.0f);
        tab[3 * dst + d] = (int)lrintf(f * 2048.0f);
    }
}

int launch_ingest_resize(hipStream_t st, const unsigned char *src, int n, int Hs, int Ws, unsigned char *dst, int Hd,
                         int Wd, const int *xt, const int *yt)
{
    if (n <= 0) return 0;
    IngestArgs a;
    a.src = src; a.dst = dst; a.n = n; a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd; a.xt = xt; a.yt = yt;
    dim3 grid((unsigned)((Wd + 255) / 256), (unsigned)Hd, (unsigned)n);
    hipLaunchKernelGGL(ingest_resize_kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
