// vrt_ray_sort_kernel.hip -- sorted bundles (vrt_hip_set_ray_sort): what runs ahead of a bundle's kernels while the switch is on.
// A wave of a lane = ray kernel visits the members of every sphere that SOME lane of it keeps, so rays that are neighbours in the
// bundle but not in space (probes, a shuffled batch) pay for each other's spheres.  A ray's bits are a function of (ray, scene,
// options), whatever its wave-mates are (vrt_ray_kernel.hip), so the library may shade a bundle in any order as long as every result
// is written at the caller's ray index.  This file gives it an order ("Sorted bundles"):
//   key    ray_sort_key_kernel: lane = ray over the bundle's own order; the sphere tests of the cull the bundle will run and nothing
//          below them (INDEXED: group spheres, the leaf spheres of the groups some lane keeps, kc = the lane's own group test && its own
//          leaf test; otherwise the chunk spheres).  first / last = the lowest / highest sphere the ray's own tests keep;
//          key[r] = min(first, 0xFFFF) << 16 | min(last, 0xFFFF), 0xFFFFFFFF for a ray that keeps none; ids[r] = r.
//          FILED in a packed form of the same order, so that the sort has fewer digits to pass over: with B = ray_sort_field_bits(spheres)
//          (the bits that hold the number of spheres itself, at most 16), first << B | last, and spheres << B | spheres for a ray
//          that keeps none -- above every other key, as 0xFFFFFFFF is.  B = 16 is the key as documented; ray_sort_unpack gives it back.
//          Like ray_short_cull, a wave visits the leaf spheres of every group that SOME lane of it keeps (the union over its lanes, in
//          the bundle's own order: this pass is not itself sorted); there is no member test.
//   sort   rocPRIM's stable radix_sort_pairs (key, ray id) over the 2 B bits of the packed key: order[slot] = ray id, ties in ray order.
// The lane = ray kernels then take their ray from order[slot] (ray_short_slot in vrt_ray_cull.hpp).  No wait, no allocation here.
#include <algorithm>
#include <cstring> // ahead of rocprim.hpp: its texture_cache_iterator.hpp uses memcpy undeclared
#include <rocprim/rocprim.hpp>

#include "vrt_ray_cull.hpp"

namespace vrtk {

struct RaySortArgs {
    RayArgs a; // first: the text of vrt_ray_cull.hpp reads it where every bundle kernel has it
    uint32_t *keys, *ids;
    unsigned long long *none;
    uint32_t field_bits, none_key; // the packed key: first << field_bits | last, none_key for a ray that keeps no sphere
};

template <bool INDEXED>
__global__ __launch_bounds__(64) void ray_sort_key_kernel(RaySortArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RaySortArgs &A = kernel_args<RaySortArgs>();
    const RayArgs &P = A.a;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r = (uint64_t)blockIdx.x * 64u + lane;
    const bool valid = r < P.nrays; // the grid has no wave without a valid ray
    const LaneRay ray = load_ray(P, valid ? r : P.nrays - 1);
    const uint32_t nch = (P.S.n + 63u) / 64u;
    uint32_t first = 0xFFFFFFFFu, last = 0u;
    if constexpr (INDEXED) {
        const uint32_t ngr = (nch + 63u) / 64u;
        for (uint32_t g = 0; g < ngr; ++g) {
            const bool kg = valid && ray_chunk_keeps(uload(P.groups, g), ray);
            if (__ballot(kg) == 0ull) continue;
            const uint32_t lf0 = g * 64u, lf1 = min(lf0 + 64u, nch);
            for (uint32_t lf = lf0; lf < lf1; ++lf) {
                if (kg && ray_chunk_keeps(uload(P.leaves, lf), ray)) { first = min(first, lf); last = lf; }
            }
        }
    } else {
        for (uint32_t c = 0; c < nch; ++c) {
            if (valid && ray_chunk_keeps(uload(P.chunks, c), ray)) { first = min(first, c); last = c; }
        }
    }
    const bool none = first == 0xFFFFFFFFu;
    if (valid) {
        A.keys[r] = none ? A.none_key : (min(first, 0xFFFFu) << A.field_bits) | min(last, 0xFFFFu);
        A.ids[r] = (uint32_t)r;
    }
    const unsigned long long without = __ballot(valid && none);
    if (lane == 0 && without) atomicAdd(A.none, (unsigned long long)__popcll(without));
}

uint32_t ray_sort_field_bits(uint32_t spheres)
{
    uint32_t b = 1;
    while (b < 16u && (spheres >> b)) ++b;
    return b;
}
static uint32_t ray_sort_none_key(uint32_t spheres, uint32_t b) { return b == 16u ? 0xFFFFFFFFu : (spheres << b) | spheres; }

uint32_t ray_sort_unpack(uint32_t packed, uint32_t spheres)
{
    const uint32_t b = ray_sort_field_bits(spheres);
    if (packed == ray_sort_none_key(spheres, b)) return 0xFFFFFFFFu;
    return ((packed >> b) << 16) | (packed & ((1u << b) - 1u));
}

size_t ray_sort_bytes(size_t nrays, uint32_t spheres)
{
    size_t bytes = 0;
    uint32_t *none = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, none, none, none, none, nrays, 0u, 2u * ray_sort_field_bits(spheres)) != hipSuccess) return 0;
    return bytes ? bytes : 1;
}

hipError_t launch_ray_sort(const RayArgs &a, bool indexed, const RaySort &o, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(o.none, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const uint32_t b = ray_sort_field_bits(o.spheres);
    RaySortArgs k{ a, o.keys, o.ids, o.none, b, ray_sort_none_key(o.spheres, b) };
    k.a.order = nullptr; // the key of ray r is filed at r
    const dim3 grid((uint32_t)((a.nrays + 63u) / 64u));
    if (indexed) hipLaunchKernelGGL(ray_sort_key_kernel<true>, grid, dim3(64), 0, st, k);
    else hipLaunchKernelGGL(ray_sort_key_kernel<false>, grid, dim3(64), 0, st, k);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = o.sort_bytes;
    return rocprim::radix_sort_pairs(o.sort_tmp, bytes, o.keys, o.keys_sorted, o.ids, o.order, (size_t)a.nrays, 0u, 2u * b, st);
}

} // namespace vrtk
