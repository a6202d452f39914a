// stream_state.hip -- the stream slots' state on its way between the table and a call (dt_track_stream_forward).
//
// The recurrent kernels address the streams of a call with ONE batch stride; the slots a call names are anywhere in the
// table.  So the call's h / c rows are gathered into contiguous buffers before step 0 and scattered back after step T - 1:
// 4 x n x G*G*U x 4 bytes per call (1.4 MB for one 416x416 stream), pure streaming.  The slot list is read from a device
// array, so the launches can live in a replayed graph while the list changes from call to call.
#include "dt_internal.h"

// 16 bytes per lane, consecutive lanes on consecutive addresses: a wavefront moves 1 KiB = eight whole 128-byte lines per
// trip (row is a multiple of 32 floats, so a row is whole lines and 16-byte aligned wherever it starts).
// grid: x = blocks per row, y = stream of the call, z = 0: h, 1: c.
__global__ __launch_bounds__(256) void stream_state_move_kernel(StateMove a)
{
    const int i = blockIdx.y, which = blockIdx.z;
    const int slot = a.slots[i];
    float4 *tab = reinterpret_cast<float4 *>((which ? a.tab_c : a.tab_h) + (long long)slot * a.row);
    float4 *buf = reinterpret_cast<float4 *>(which ? a.c + (long long)i * a.c_bs : a.h + (long long)i * a.h_bs);
    const int n4 = a.row >> 2, stride = gridDim.x * 256;
    int *frames = a.meta + slot * STREAM_META + SM_FRAMES;
    if (a.scatter) {
        for (int q = blockIdx.x * 256 + threadIdx.x; q < n4; q += stride) tab[q] = buf[q];
        if (which == 0 && blockIdx.x == 0 && threadIdx.x == 0) {      // (no launch reads the counter while this one writes it)
            const int f = *frames;
            *frames = f > (1 << 30) ? f : f + a.T;                    // saturates: only "zero or not" is ever read
        }
    } else {
        const bool fresh = *frames == 0;      // a fresh slot's rows are whatever an earlier stream left there: they read as zeros
        for (int q = blockIdx.x * 256 + threadIdx.x; q < n4; q += stride) buf[q] = fresh ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : tab[q];
    }
}

int launch_stream_state_move(hipStream_t st, const StateMove &a)
{
    if (a.n <= 0) return 0;
    if (a.row <= 0 || a.row % 32 || a.n > 65535) return 2;
    const int n4 = a.row / 4;
    int bx = (n4 + 1023) / 1024;      // four trips per thread: 44 workgroups for one 416x416 stream, 2112 for 48
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(stream_state_move_kernel, dim3((unsigned)bx, (unsigned)a.n, 2u), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---------------------------------------------------------------------------
// the slot list of a call: host numbers -> device list, 64 per launch, as kernel arguments
// ---------------------------------------------------------------------------
struct SlotChunk { int v[64]; };

__global__ __launch_bounds__(64) void stream_slots_kernel(SlotChunk c, int count, int *dst, int *reset_meta)
{
    const int lane = threadIdx.x;
    if (lane >= count) return;
    const int slot = c.v[lane];
    dst[lane] = slot;
    if (reset_meta) *reinterpret_cast<int4 *>(reset_meta + slot * STREAM_META) = make_int4(0, 0, 0, 0);
}

int launch_stream_slots(hipStream_t st, const int *h_slots, int n, int *d_list, int *reset_meta)
{
    static_assert(STREAM_META == 4, "a meta row is one int4");
    for (int base = 0; base < n; base += 64) {
        SlotChunk c;
        const int count = n - base < 64 ? n - base : 64;
        for (int j = 0; j < 64; ++j) c.v[j] = j < count ? h_slots[base + j] : 0;
        hipLaunchKernelGGL(stream_slots_kernel, dim3(1), dim3(64), 0, st, c, count, d_list + base, reset_meta);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    return 0;
}

// the listed slots' velocity stamps: zero = the slot's stored velocities belong to no table (dt_internal.h:AssocCarry)
__global__ __launch_bounds__(256) void stream_clear_stamps_kernel(const int *list, int n, int *vstamp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) vstamp[list[i]] = 0;
}

int launch_stream_clear_stamps(hipStream_t st, const int *d_list, int n, int *vstamp)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(stream_clear_stamps_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_list, n, vstamp);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
