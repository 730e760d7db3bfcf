// vrt_ray_plan_kernel.hip -- ray plans (vrt_hip_ray_plan_create*): the cull of a bundle run once and KEPT.  A plan is made in the count,
// scan, wait, fill shape of the ordered gradient tables:
//   count    ray_count_kernel and rocPRIM's exclusive scan (launch_grad_ordered_count of vrt_grad_ordered_kernel.hip, not written again):
//            len[r] = the list length of ray r, long rays too; off[r] = where its list begins; the total for the host
//   info     ray_plan_info_kernel: from the lengths alone the rays with a list longer than RAY_PL (the long kernel's queue), those beyond
//            RAY_LCAP and the longest list -- read back with the total in the one wait, so that the queue and the lists get their size
//   fill     an eighth kernel pair on the skeleton of vrt_ray_cull.hpp, the text every bundle runs: the lane = ray kernel culls and copies
//            its lane's list out of s_list; one wave per long ray re-culls and copies the LDS and scratch-slot list.  The short kernel
//            files the long rays into the PLAN's queue as it files them into the context's for a bundle.
// The lists are the bundles' lists because they are made by the bundles' text: ascending scene order, the same rays long.  A planned bundle
// (the RAY_LIST_PLAN instantiations of the seven units) reads them back through ray_short_begin / ray_long_next and tests nothing.
// A ray whose fill finds another length than its count writes NOTHING (its range belongs to that length) and is counted: the host refuses
// such a plan.  Plain vector loads and stores; integer atomics for the words.
#include "vrt_ray_cull.hpp"

namespace vrtk {

__global__ __launch_bounds__(256) void ray_plan_info_kernel(const uint32_t *__restrict__ len, uint64_t nrays, unsigned long long *__restrict__ words)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t l = i < nrays ? len[i] : 0u;
    const uint32_t longest = wave_max_u32(l); // the whole wave is here: no return above
    if (l > (uint32_t)RAY_PL) atomicAdd(&words[RAY_PLAN_LONG], 1ull);
    if (l > (uint32_t)RAY_LCAP) atomicAdd(&words[RAY_PLAN_SCRATCH], 1ull);
    if ((threadIdx.x & 63u) == 0u && longest) atomicMax(&words[RAY_PLAN_LONGEST], (unsigned long long)longest);
}

template <int SRC>
__global__ __launch_bounds__(64) void ray_plan_fill_short_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    const uint32_t lane = threadIdx.x & 63u;
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane); // the cull, and the long rays into the plan's queue
    if (!R.writes) return; // a long ray's list is its wave's to copy
    if (R.nl != P.pl_len[R.rc]) { atomicAdd(&P.pl_words[RAY_PLAN_MISMATCH], 1ull); return; }
    uint32_t *mine = P.pl_fill + P.pl_off[R.rc];
    for (uint32_t k = 0; k < R.nl; ++k) mine[k] = s_list[k * 64u + lane];
}

template <int SRC>
__global__ __launch_bounds__(64) void ray_plan_fill_long_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    LongRay L = ray_long_begin<SRC>(&P);
    while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) {
        if (L.n != P.pl_len[L.r]) { // wave-uniform
            if (lane == 0) atomicAdd(&P.pl_words[RAY_PLAN_MISMATCH], 1ull);
            continue;
        }
        uint32_t *its = P.pl_fill + P.pl_off[L.r];
        for (uint32_t p = lane; p < L.n; p += 64u) its[p] = long_list_entry(s_list, L.slot, p);
    }
}

hipError_t launch_ray_plan_info(const uint32_t *len, uint64_t nrays, unsigned long long *words, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(words + GRAD_ORD_WORDS, 0, (RAY_PLAN_WORDS - GRAD_ORD_WORDS) * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ray_plan_info_kernel, dim3((uint32_t)((nrays + 255u) / 256u)), dim3(256), 0, st, len, nrays, words);
    return hipGetLastError();
}

void launch_ray_plan_fill(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    if (!a.nrays || !long_grid) return;
    if (src == RAY_LIST_INDEX) launch_ray_kernels(ray_plan_fill_short_kernel<RAY_LIST_INDEX>, ray_plan_fill_long_kernel<RAY_LIST_INDEX>, a, long_grid, st);
    else launch_ray_kernels(ray_plan_fill_short_kernel<RAY_LIST_CHUNKS>, ray_plan_fill_long_kernel<RAY_LIST_CHUNKS>, a, long_grid, st);
}

} // namespace vrtk
