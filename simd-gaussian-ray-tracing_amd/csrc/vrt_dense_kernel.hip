// vrt_dense_kernel.hip -- the exact dense kernel (single frame and frame batch) around dense_shade_block (vrt_dense_block.hpp, which the
// table kernel shares), and order_dense, which sorts its queue.  This unit is most of the library's compile time: 74 instantiations.
#include "vrt_dense_block.hpp"

namespace vrtk {

// The exact dense kernel: persistent DW-wave workgroups pull blocks (the cells of the dense queue, then what the block kernel handed
// over) with one atomic per block and shade them with dense_shade_block (vrt_dense_block.hpp).
template <int EXP, int ERF, int EC, int DW, bool SKIP = true>
__device__ __forceinline__ void render_dense_body(const SceneTables &S, const TileLists &T, const CellGrid &C, const RayGen &R,
                                                  const RenderTarget &O)
{
    __shared__ DenseLds<DW> lds;
    __shared__ uint32_t s_item;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t n_dense16 = *C.n_dense * 16u, n_items = n_dense16 + *C.n_overflow;
    if (C.feedback && blockIdx.x == 0 && tid == 0) { // launch feedback: how much this frame had for this kernel
        __hip_atomic_store(&C.feedback[2], n_items, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&C.feedback[3], C.frame_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const uint32_t *dense_queue = C.dense_is_sorted ? C.dense_sorted : C.dense;
    uint32_t *scratch = C.scratch + (size_t)blockIdx.x * C.cstride;
    const unsigned long long t_start = O.stats ? wall_clock64() : 0ull;
    DenseVisits visits;

    for (;;) {
        __syncthreads(); // everyone is done with the previous item's LDS
        if (tid == 0) s_item = atomicAdd(C.dense_next, 1u);
        __syncthreads();
        const uint32_t item = s_item;
        if (item >= n_items) {
            if (O.stats && lane == 0) {
                atomicAdd(&O.stats[STAT_DENSE_VISITS_FULL], (unsigned long long)visits.full); atomicAdd(&O.stats[STAT_DENSE_VISITS_ZERO], (unsigned long long)visits.zero);
                atomicAdd(&O.stats[STAT_DENSE_VISITS_COMMON], (unsigned long long)visits.common);
            }
            if (O.stats && tid == 0) { // workgroup timeline: how long the queue kept this workgroup busy
                const unsigned long long t_end = wall_clock64();
                atomicMin(&O.stats[STAT_DENSE_T_FIRST], t_start); atomicMax(&O.stats[STAT_DENSE_T_LAST], t_end);
                atomicAdd(&O.stats[STAT_DENSE_BUSY_TICKS], t_end - t_start); atomicAdd(&O.stats[STAT_DENSE_WORKGROUPS], 1ull);
            }
            break;
        }
        uint32_t cell, bi;
        if (item < n_dense16) { cell = dense_queue[item >> 4]; bi = item & 15u; }
        else { const uint32_t packed = C.overflow[item - n_dense16]; cell = packed >> 4; bi = packed & 15u; }
        dense_shade_block<EXP, ERF, EC, DW, SKIP>(S, T, C, R, O, lds, scratch, cell, bi, item < n_dense16, visits);
    }
}
template <int EXP, int ERF, int EC, int DW, bool SKIP = true>
__global__ __launch_bounds__(DW * 64, 4) void render_dense_kernel(RenderArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RenderArgs &a = kernel_args<RenderArgs>();
    render_dense_body<EXP, ERF, EC, DW, SKIP>(a.S, a.T, a.C, a.R, a.O);
}
template <int EXP, int ERF, int EC, int DW, bool SKIP = true>
__global__ __launch_bounds__(DW * 64, 4) void render_dense_batch_kernel(const FrameArgs *__restrict__ frames)
{
    const FrameArgs &a = frames[blockIdx.y];
    render_dense_body<EXP, ERF, EC, DW, SKIP>(a.S, a.T, a.C, a.R, a.O);
}

// Queue order of the dense kernel: cells by descending candidate count (a block costs ~ count^2), so that the
// blocks still running when the queue empties are the cheapest ones.  Counting sort, one workgroup.
__device__ __forceinline__ void order_dense_body(const CellGrid &C)
{
    __shared__ uint32_t s_hist[1024], s_scan[1024];
    const uint32_t n = *C.n_dense, tid = threadIdx.x;
    s_hist[tid] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 1024) atomicAdd(&s_hist[1023u - (min(C.count[C.dense[i]], 4095u) >> 2)], 1u);
    __syncthreads();
    // exclusive prefix over the buckets (bucket 0 = longest lists)
    uint32_t v = s_hist[tid];
    s_scan[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t add = tid >= off ? s_scan[tid - off] : 0u;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    s_hist[tid] = s_scan[tid] - v;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 1024) {
        const uint32_t cell = C.dense[i];
        C.dense_sorted[atomicAdd(&s_hist[1023u - (min(C.count[cell], 4095u) >> 2)], 1u)] = cell;
    }
}

__global__ __launch_bounds__(1024) void order_dense_kernel(CellGrid C) { order_dense_body(C); }
__global__ __launch_bounds__(1024) void order_dense_batch_kernel(const FrameArgs *__restrict__ frames)
{
    const FrameArgs &a = frames[blockIdx.x];
    if (a.do_order) order_dense_body(a.C);
}
void launch_order_dense(const CellGrid &c, hipStream_t st)
{
    hipLaunchKernelGGL(order_dense_kernel, dim3(1), dim3(1024), 0, st, c);
}
void launch_order_dense_batch(const FrameArgs *d_frames, const FrameArgs *h_frames, uint32_t nframes, hipStream_t st)
{
    bool any = false;
    for (uint32_t f = 0; f < nframes; ++f) any = any || h_frames[f].do_order;
    if (any) hipLaunchKernelGGL(order_dense_batch_kernel, dim3(nframes), dim3(1024), 0, st, d_frames);
}

template <int EXP, int ERF>
static void launch_render_dense_t(const SceneTables &s, const TileLists &t, const CellGrid &c, const RayGen &r,
                                  const RenderTarget &o, uint32_t grid, int dw, hipStream_t st)
{
    if (grid == 0) return;
    if (dw == 17) hipLaunchKernelGGL((render_dense_kernel<EXP, ERF, 6, 16, false>), dim3(grid), dim3(1024), 0, st, RenderArgs{ s, t, c, r, o });
    else if (dw == 16) hipLaunchKernelGGL((render_dense_kernel<EXP, ERF, 6, 16>), dim3(grid), dim3(1024), 0, st, RenderArgs{ s, t, c, r, o });
    else if (dw == 8) hipLaunchKernelGGL((render_dense_kernel<EXP, ERF, 6, 8>), dim3(grid), dim3(512), 0, st, RenderArgs{ s, t, c, r, o });
    else hipLaunchKernelGGL((render_dense_kernel<EXP, ERF, 6, 4>), dim3(grid), dim3(256), 0, st, RenderArgs{ s, t, c, r, o });
}
void launch_render_dense(const SceneTables &s, const TileLists &t, const CellGrid &c, const RayGen &r,
                         const RenderTarget &o, uint32_t grid, int dw, int exp_kind, int erf_kind, hipStream_t st)
{
    VRT_DISPATCH_EXP_ERF(launch_render_dense_t, s, t, c, r, o, grid, dw, st);
}
template <int EXP, int ERF>
static void launch_render_dense_batch_t(const FrameArgs *d_frames, uint32_t nframes, uint32_t grid, int dw, hipStream_t st)
{
    if (grid == 0 || nframes == 0) return;
    const dim3 g(grid, nframes);
    if (dw == 17) hipLaunchKernelGGL((render_dense_batch_kernel<EXP, ERF, 6, 16, false>), g, dim3(1024), 0, st, d_frames);
    else if (dw == 16) hipLaunchKernelGGL((render_dense_batch_kernel<EXP, ERF, 6, 16>), g, dim3(1024), 0, st, d_frames);
    else if (dw == 8) hipLaunchKernelGGL((render_dense_batch_kernel<EXP, ERF, 6, 8>), g, dim3(512), 0, st, d_frames);
    else hipLaunchKernelGGL((render_dense_batch_kernel<EXP, ERF, 6, 4>), g, dim3(256), 0, st, d_frames);
}
void launch_render_dense_batch(const FrameArgs *d_frames, uint32_t nframes, uint32_t grid, int dw, int exp_kind, int erf_kind,
                               hipStream_t st)
{
    VRT_DISPATCH_EXP_ERF(launch_render_dense_batch_t, d_frames, nframes, grid, dw, st);
}
} // namespace vrtk
