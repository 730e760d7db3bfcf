// vrt_grad_ordered_kernel.hip -- ordered gradient tables (vrt_hip_set_grad_ordered): what stands around the record kernels of
// vrt_ray_grad_ordered_kernel.hip and vrt_ray_trans_grad_ordered_kernel.hip.  An ordered gradient bundle adds nothing to the caller's
// table while its rays are shaded: every row segment a ray would add is STORED as a record (Gaussian index, ray id, 9 floats = the
// table's columns 0..8), and one reduction sums each Gaussian's records in a fixed order ("Ordered gradient
// tables").  This file has
//   count    ray_count_kernel: the lane = ray cull alone (ray_short_cull, the text every bundle runs), len[r] = the list length, which runs
//            on past RAY_PL: the full length of a long ray's list too.  Files nothing into the queue, counts no statistics.
//   place    rows[r] (by the count kernel: len, or 2 len for a long ray of the radiance gradient), an exclusive scan in ray order
//            (rocPRIM, 64-bit sums) = base[r], and the total for the host
//   sort     rocPRIM's stable radix_sort_pairs, key = Gaussian index on ceil(log2(N + 1)) bits (N = the key of a sentinel row, sorted last),
//            value = record position: the consumed order is (Gaussian, ray id, the record's place in its ray)
//   reduce   one wave per Gaussian with records.  NORMATIVE, per column c over the records rho_0 .. rho_{m-1} of the Gaussian in consumed
//            order: lane l holds a_l = (((+0 + rho_l[c]) + rho_{l+64}[c]) + rho_{l+128}[c]) + ..., a lane without a record +0; then six steps
//            s = 1, 2, 4, 8, 16, 32, each a_l <- a_l + a_{l xor s} from the values before the step; then table[j, c] <- table[j, c] + a_0.
//            Plain float32 adds.  Rows of Gaussians without records, columns 9..11 and (FIRST = 4) columns 0..3 are not written at all.
// No float atomic anywhere; the words of the statistics are integer atomics.
#include <algorithm>
#include <cstring> // ahead of rocprim.hpp: its texture_cache_iterator.hpp uses memcpy undeclared
#include <rocprim/rocprim.hpp>

#include "vrt_ray_cull.hpp"

namespace vrtk {

template <int SRC>
__global__ __launch_bounds__(64) void ray_count_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // the cull files a short list here; nobody reads it
    const uint32_t lane = threadIdx.x & 63u;
    const ShortSlot slot = ray_short_slot(&P, lane); // the waves of the record kernels behind this one: a sorted bundle is counted in its sorted order
    const uint64_t r = slot.r;
    const bool valid = slot.valid;
    uint32_t nl;
    if constexpr (SRC == RAY_LIST_PLAN) nl = valid ? P.pl_len[slot.rc] : 0u; // a ray plan is bound: its lengths are the count
    else {
        const LaneRay ray = load_ray(P, slot.rc);
        const uint32_t N = S.n, nch = (N + 63u) / 64u;
        RayCullCounts cnt;
        nl = ray_short_cull<SRC>(&P, &S, N, nch, s_list, lane, valid, ray, cnt);
    }
    if (valid) {
        P.ord_len[r] = nl;
        P.ord_count[r] = (unsigned long long)nl * (nl > (uint32_t)RAY_PL && P.ord_two ? 2ull : 1ull);
    }
}

__global__ void grad_ordered_total_kernel(const unsigned long long *count, const unsigned long long *base, uint64_t nrays, unsigned long long *words)
{
    words[GRAD_ORD_TOTAL] = base[nrays - 1] + count[nrays - 1];
}

__global__ __launch_bounds__(256) void grad_ordered_iota_kernel(uint32_t *p, uint64_t from, uint64_t to)
{
    const uint64_t i = from + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < to) p[i] = (uint32_t)i;
}

// seg[2 j], seg[2 j + 1]: where Gaussian j's records begin and end in the sorted order (both 0, cleared on the stream before: none)
__global__ __launch_bounds__(256) void grad_ordered_heads_kernel(uint64_t total, uint32_t N, const uint32_t *__restrict__ keys, uint32_t *__restrict__ seg)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint32_t k = keys[i];
    if (k >= N) return; // a sentinel row: read by no segment
    if (i == 0 || keys[i - 1] != k) seg[2 * (size_t)k] = (uint32_t)i;
    if (i + 1 == total || keys[i + 1] != k) seg[2 * (size_t)k + 1] = (uint32_t)(i + 1);
}

// One wave per Gaussian, four to a workgroup.  FIRST: the first column reduced (0: radiance gradient, 4: transmittance gradient).
template <int FIRST>
__global__ __launch_bounds__(256) void grad_ordered_reduce_kernel(uint32_t N, const uint32_t *__restrict__ seg, const uint32_t *__restrict__ order,
                                                                  const float *__restrict__ rows, float *__restrict__ table,
                                                                  unsigned long long *__restrict__ words)
{
    constexpr int NC = GRAD_ORD_COLS - FIRST;
    const uint32_t lane = threadIdx.x & 63u, j = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (j >= N) return; // wave-uniform, as everything below
    const uint32_t s0 = seg[2 * (size_t)j], s1 = seg[2 * (size_t)j + 1];
    if (s1 <= s0) return;
    const uint64_t m = s1 - s0;
    float a[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = 0.f;
    for (uint64_t k = lane; k < m; k += 64u) {
        const float *row = rows + (size_t)order[s0 + k] * GRAD_ORD_COLS + FIRST;
#pragma unroll
        for (int c = 0; c < NC; ++c) a[c] = add_ref(a[c], row[c]);
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1)
#pragma unroll
        for (int c = 0; c < NC; ++c) a[c] = add_ref(a[c], __shfl_xor(a[c], s, 64));
    if (lane == 0) {
        float *out = table + (size_t)j * VRT_HIP_GRAD_STRIDE + FIRST;
#pragma unroll
        for (int c = 0; c < NC; ++c) out[c] = add_ref(out[c], a[c]);
        atomicAdd(&words[GRAD_ORD_RECORDS], (unsigned long long)m);
        atomicAdd(&words[GRAD_ORD_TOUCHED], 1ull);
        atomicMax(&words[GRAD_ORD_LONGEST], (unsigned long long)m);
    }
}

size_t grad_ordered_scan_bytes(size_t nrays)
{
    size_t bytes = 0;
    unsigned long long *none = nullptr;
    if (rocprim::exclusive_scan(nullptr, bytes, none, none, 0ull, nrays, rocprim::plus<unsigned long long>()) != hipSuccess) return 0;
    return bytes ? bytes : 1;
}

hipError_t launch_grad_ordered_count(const RayArgs &a, int src, unsigned long long *base, void *tmp, size_t tmp_bytes, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(a.ord_words, 0, GRAD_ORD_WORDS * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const dim3 grid((uint32_t)((a.nrays + 63u) / 64u));
    if (src == RAY_LIST_PLAN) hipLaunchKernelGGL(ray_count_kernel<RAY_LIST_PLAN>, grid, dim3(64), 0, st, a);
    else if (src == RAY_LIST_INDEX) hipLaunchKernelGGL(ray_count_kernel<RAY_LIST_INDEX>, grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL(ray_count_kernel<RAY_LIST_CHUNKS>, grid, dim3(64), 0, st, a);
    e = rocprim::exclusive_scan(tmp, tmp_bytes, a.ord_count, base, 0ull, (size_t)a.nrays, rocprim::plus<unsigned long long>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grad_ordered_total_kernel, dim3(1), dim3(1), 0, st, a.ord_count, base, a.nrays, a.ord_words);
    return hipGetLastError();
}

static unsigned key_bits(uint32_t n) // ceil(log2(n + 1)): the bits of the largest key, n itself
{
    unsigned b = 1;
    while (b < 32 && (n >> b)) ++b;
    return b;
}

size_t grad_ordered_sort_bytes(uint64_t total, uint32_t n)
{
    size_t bytes = 0;
    uint32_t *none = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, none, none, none, none, (size_t)total, 0u, key_bits(n)) != hipSuccess) return 0;
    return bytes ? bytes : 1;
}

void launch_grad_ordered_iota(uint32_t *p, uint64_t from, uint64_t to, hipStream_t st)
{
    if (to > from) hipLaunchKernelGGL(grad_ordered_iota_kernel, dim3((uint32_t)((to - from + 255u) / 256u)), dim3(256), 0, st, p, from, to);
}

hipError_t launch_grad_ordered_reduce(const GradOrderedSort &o, hipStream_t st)
{
    size_t bytes = o.sort_bytes;
    hipError_t e = rocprim::radix_sort_pairs(o.sort_tmp, bytes, o.keys, o.keys_sorted, o.iota, o.order, (size_t)o.total, 0u, key_bits(o.n), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(o.seg, 0, 2 * (size_t)o.n * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grad_ordered_heads_kernel, dim3((uint32_t)((o.total + 255u) / 256u)), dim3(256), 0, st, o.total, o.n, o.keys_sorted, o.seg);
    const dim3 grid((o.n + 3u) / 4u);
    if (o.first_col == 0)
        hipLaunchKernelGGL(grad_ordered_reduce_kernel<0>, grid, dim3(256), 0, st, o.n, o.seg, o.order, o.rows, o.table, o.words);
    else
        hipLaunchKernelGGL(grad_ordered_reduce_kernel<4>, grid, dim3(256), 0, st, o.n, o.seg, o.order, o.rows, o.table, o.words);
    return hipGetLastError();
}

} // namespace vrtk
