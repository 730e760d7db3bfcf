// vrt_scene_kernel.hip -- a scene set from device memory (vrt_hip_set_gaussians_device): the ingest kernel that turns the caller's packed
// rows into the nine SoA columns and reduces albedo_scale, and the Morton index of the ray bundles built on the device -- bounding box,
// keys, a stable radix sort, the permuted rows and the open leaves.  It reproduces morton_order / build_ray_index (vrt_hip_rays.cpp)
// bit for bit: the same double-precision key, the same order among equal keys, the same NaN radius for a leaf with a member that is
// not finite.  The sort is rocPRIM's radix_sort_pairs (header-only: the library still links only libamdhip64).
#include <algorithm>
#include <cstring> // ahead of rocprim.hpp: its texture_cache_iterator.hpp uses memcpy undeclared
#include <rocprim/rocprim.hpp>

#include "vrt_kernels_common.hpp"

namespace vrtk {

// ---------------------------------------------------------------------------------------------
// Ingest: one thread per Gaussian.  mu [n, 3], albedo [n, 4] (column 3 = alpha), sigma [n], mag [n] -> columns mu_x mu_y mu_z ar ag ab
// aa sigma mag.  albedo_scale: the largest finite |albedo| over the four channels; the bit patterns of non-negative floats order as
// unsigned integers, so the maximum is taken on them -- over the wave on the DPP path, then one atomicMax per wave, and only by a wave
// that holds a value above 1 (the host takes max(1, word): a scene in the reference's range issues no atomic at all).
// ---------------------------------------------------------------------------------------------
template <bool ALIGNED>
__global__ __launch_bounds__(256) void ingest_scene_kernel(uint32_t n, const float *__restrict__ mu, const float *__restrict__ albedo,
                                                           const float *__restrict__ sigma, const float *__restrict__ mag, SceneColumns out,
                                                           uint32_t *__restrict__ albedo_bits)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t m = 0;
    if (i < n) { // (no early return: the reduction below is over a full wave)
        float4 a;
        if (ALIGNED) a = reinterpret_cast<const float4 *>(albedo)[i];
        else a = make_float4(albedo[4 * i], albedo[4 * i + 1], albedo[4 * i + 2], albedo[4 * i + 3]);
        out.c[0][i] = mu[3 * i]; out.c[1][i] = mu[3 * i + 1]; out.c[2][i] = mu[3 * i + 2];
        out.c[3][i] = a.x; out.c[4][i] = a.y; out.c[5][i] = a.z; out.c[6][i] = a.w;
        out.c[7][i] = sigma[i]; out.c[8][i] = mag[i];
        const uint32_t b[4] = { __float_as_uint(a.x) & 0x7FFFFFFFu, __float_as_uint(a.y) & 0x7FFFFFFFu, __float_as_uint(a.z) & 0x7FFFFFFFu,
                                __float_as_uint(a.w) & 0x7FFFFFFFu };
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (b[k] < 0x7F800000u) m = max(m, b[k]); // NaN and inf are not counted
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63u) == 0 && m > 0x3F800000u) atomicMax(albedo_bits, m);
}

void launch_ingest_scene(uint32_t n, const float *mu, const float *albedo, const float *sigma, const float *mag, const SceneColumns &out,
                         uint32_t *albedo_bits, hipStream_t st)
{
    if (!n) return;
    const dim3 grid((uint32_t)(((uint64_t)n + 255u) / 256u));
    if (((uintptr_t)albedo & 15u) == 0)
        hipLaunchKernelGGL(ingest_scene_kernel<true>, grid, dim3(256), 0, st, n, mu, albedo, sigma, mag, out, albedo_bits);
    else
        hipLaunchKernelGGL(ingest_scene_kernel<false>, grid, dim3(256), 0, st, n, mu, albedo, sigma, mag, out, albedo_bits);
}

// ---------------------------------------------------------------------------------------------
// Morton index.  box[0..2]: maximum of ~code(v) over the finite centres (the lowest x, y, z), box[3..5]: maximum of code(v) (the
// highest), code = the float's bits mapped so that unsigned order is numeric order.  Cleared to 0 on the stream ahead of the reduction:
// no code and no complement of one is 0 for a finite float, so 0 = no finite centre.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t order_code(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_decode(uint32_t c)
{
    return __uint_as_float((c & 0x80000000u) ? (c & 0x7FFFFFFFu) : ~c);
}
__device__ __forceinline__ bool finite_centre(const float4 &p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

__global__ __launch_bounds__(256) void morton_box_kernel(uint32_t n, const float4 *__restrict__ mu_sig, uint32_t *__restrict__ box)
{
    uint32_t lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const float4 p = mu_sig[i];
        if (!finite_centre(p)) continue;
        const uint32_t c[3] = { order_code(p.x), order_code(p.y), order_code(p.z) };
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = max(lo[a], ~c[a]); hi[a] = max(hi[a], c[a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint32_t l = wave_max_u32(lo[a]), h = wave_max_u32(hi[a]);
        if ((threadIdx.x & 63u) == 0 && h) { atomicMax(&box[a], l); atomicMax(&box[3 + a], h); }
    }
}

// 10 bits spread to every third bit
__device__ __forceinline__ uint32_t spread3(uint32_t v)
{
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// key[i]: the centre quantised to 10 bits per axis over the box, in double precision as morton_order does it (an axis of no extent,
// or of no finite centre: 0), x in the lowest bit of every triple; a centre that is not finite: 0
__global__ __launch_bounds__(256) void morton_keys_kernel(uint32_t n, const float4 *__restrict__ mu_sig, const uint32_t *__restrict__ box,
                                                          uint32_t *__restrict__ keys)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 p = mu_sig[i];
    uint32_t k = 0;
    if (finite_centre(p)) {
        const float v[3] = { p.x, p.y, p.z };
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t cl = box[a], ch = box[3 + a];
            const double lo = cl ? (double)order_decode(~cl) : (double)INFINITY, hi = ch ? (double)order_decode(ch) : -(double)INFINITY;
            const double ext = hi - lo;
            const uint32_t q = ext > 0.0 ? (uint32_t)fmin(1023.0, floor(((double)v[a] - lo) / ext * 1024.0)) : 0u;
            k |= spread3(q) << a;
        }
    }
    keys[i] = k;
}

// the rows of the tables in Morton order
__global__ __launch_bounds__(256) void morton_gather_kernel(uint32_t n, const uint32_t *__restrict__ perm, const float4 *__restrict__ mu_sig,
                                                            const float4 *__restrict__ gB, float4 *__restrict__ mu_sig_m, float4 *__restrict__ gB_m)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = perm[p];
    mu_sig_m[p] = mu_sig[i];
    gB_m[p] = gB[i];
}

// The chunk kernel's minima and maxima pass over a NaN: a member whose centre or reach is not finite would sit outside its leaf's sphere,
// yet the member test keeps it.  Such a leaf gets a NaN radius, which keeps (build_ray_index has the rule).  Every such member of a leaf
// stores the same word.
__global__ __launch_bounds__(256) void morton_open_leaves_kernel(uint32_t n, const float4 *__restrict__ mu_sig_m, const float4 *__restrict__ gB_m,
                                                                 float4 *__restrict__ leaves)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const float4 m = mu_sig_m[p], b = gB_m[p];
    const bool ok = finite_centre(m) && !isnan(b.y) && !isnan(b.w) && b.w < INFINITY;
    if (!ok) leaves[p / 64u].w = __uint_as_float(0x7FC00000u);
}

size_t morton_sort_bytes(uint32_t n)
{
    size_t bytes = 0;
    uint32_t *none = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, none, none, none, none, (size_t)n, 0u, 30u) != hipSuccess) return 0;
    return bytes ? bytes : 1;
}

hipError_t launch_morton_index(uint32_t n, const float4 *mu_sig, const float4 *gB, const uint32_t *iota, uint32_t *box, uint32_t *keys /* 2 n */,
                               void *sort_tmp, size_t sort_bytes, uint32_t *perm, float4 *mu_sig_m, float4 *gB_m, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipError_t e = hipMemsetAsync(box, 0, 6 * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + 255u) / 256u);
    hipLaunchKernelGGL(morton_box_kernel, dim3(std::min(blocks, 2048u)), dim3(256), 0, st, n, mu_sig, box);
    hipLaunchKernelGGL(morton_keys_kernel, dim3(blocks), dim3(256), 0, st, n, mu_sig, box, keys);
    // (key, scene index) pairs, stable over the 30 bits of a key: ties stay in scene order, as std::stable_sort leaves them
    e = rocprim::radix_sort_pairs(sort_tmp, sort_bytes, keys, keys + n, iota, perm, (size_t)n, 0u, 30u, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(morton_gather_kernel, dim3(blocks), dim3(256), 0, st, n, perm, mu_sig, gB, mu_sig_m, gB_m);
    return hipGetLastError();
}

void launch_morton_open_leaves(uint32_t n, const float4 *mu_sig_m, const float4 *gB_m, float4 *leaves, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(morton_open_leaves_kernel, dim3((uint32_t)(((uint64_t)n + 255u) / 256u)), dim3(256), 0, st, n, mu_sig_m, gB_m, leaves);
}

} // namespace vrtk
