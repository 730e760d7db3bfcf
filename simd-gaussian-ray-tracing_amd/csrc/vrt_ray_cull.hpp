// vrt_ray_cull.hpp -- the skeleton of the ray bundles, shared by vrt_ray_kernel.hip (radiance), vrt_ray_trans_kernel.hip
// (transmittance), vrt_ray_depth_kernel.hip (depth), vrt_ray_grad_kernel.hip (gradient), vrt_ray_trans_grad_kernel.hip (transmittance
// gradient), vrt_ray_tangent_kernel.hip (tangent) and vrt_ray_trans_tangent_kernel.hip (transmittance tangent): the sphere and member tests, the lane = ray cull into per-lane lists in LDS, the
// one-wave-per-ray re-cull into LDS + scratch slot, both with and without the Morton index, the queue of the long rays and the
// statistics words; around them what every kernel pair does before its own middle -- ray_short_begin (a lane's ray, list and filing),
// ray_long_begin / ray_long_next (a wave's claims of the queue, each with its re-cull) -- and launch_ray_kernels behind them.  One text
// for all seven translation units: the same rays keep the same Gaussians, go to the same kernel and count the same statistics.
// Where the lists come from is a template value of everything here (SRC, a RayListSource of vrt_kernels.h): the cull against the chunk
// spheres, the same cull through the Morton index, or the lists of a ray plan (vrt_hip_set_ray_plan; vrt_ray_plan_kernel.hip makes them
// with this very text), which are loaded and copied where the other two test -- a value and not a branch on a kernel argument, so that
// the instantiations that cull keep the machine code they had.
#pragma once
#include "vrt_kernels_common.hpp"

namespace vrtk {

// The chunk's sphere (centre, radius incl. its members' reach: build_chunks_kernel) against the LINE of one ray.  A member
// is kept by the ray criterion only within its reach of the line, and the distance to a line is 1-Lipschitz in the point,
// so a line farther than the radius from the centre keeps no member.  The d^2 - t^2 cancellation is guarded on the keeping
// side, as in chunk_keeps.  Unfused: both kernels must decide alike.
__device__ __forceinline__ bool ray_chunk_keeps(float4 ch, const LaneRay &ray)
{
    const float ax = sub_ref(ch.x, ray.ox), ay = sub_ref(ch.y, ray.oy), az = sub_ref(ch.z, ray.oz);
    const float d2 = dot3_ref(ax, ay, az, ax, ay, az);
    const float t = dot3_ref(ax, ay, az, ray.nx, ray.ny, ray.nz);
    const float dperp = __builtin_sqrtf(fmaxf(0.f, sub_ref(sub_ref(d2, mul_ref(t, t)), mul_ref(8e-6f, d2))));
    return !(mul_ref(dperp, 0.9999f) > ch.w);
}
// x = (|oc|^2 - mubar^2) / (2 sigma^2) of one ray and one Gaussian in the reference's order (ray_gaussian<false>); kept iff !(x > cull_x)
__device__ __forceinline__ bool ray_member_keeps(float4 ms, float4 bq, const LaneRay &ray)
{
    const float cx = ms.x - ray.ox, cy = ms.y - ray.oy, cz = ms.z - ray.oz;
    const float mubar = dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz);
    const float x = mul_ref(sub_ref(dot3_ref(cx, cy, cz, cx, cy, cz), mul_ref(mubar, mubar)), bq.y);
    return !(x > bq.w);
}

// A list in LDS keeps its address space through the functions below: as a plain pointer next to a scratch slot's, the two stores of
// "LDS or slot" become one store through a generic pointer.
typedef uint32_t __attribute__((address_space(3))) lds_u32;

// Uniform (scalar) 4-byte load, as uload
typedef const uint32_t __attribute__((address_space(4))) *cu32ptr;
__device__ __forceinline__ uint32_t uload_u32(const uint32_t *base, uint32_t idx) { return ((cu32ptr)(const void *)base)[idx]; }

__device__ __forceinline__ LaneRay load_ray(const RayArgs &P, uint64_t r)
{
    const uint64_t ro = P.origin_per_ray ? r : 0ull;
    LaneRay ray;
    ray.ox = P.origins[3 * ro]; ray.oy = P.origins[3 * ro + 1]; ray.oz = P.origins[3 * ro + 2];
    ray.nx = P.dirs[3 * r]; ray.ny = P.dirs[3 * r + 1]; ray.nz = P.dirs[3 * r + 2];
    return ray;
}

// sum over the 64 lanes of a full wave in a fixed order, on the DPP path (wave_inclusive_sum's steps on floats; zeros are shifted in)
#define VRT_DPP_ZERO(v, ctrl, rows, bound) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rows, 0xf, bound))
__device__ __forceinline__ float wave_sum(float v)
{
    v = add_ref(v, VRT_DPP_ZERO(v, 0x111, 0xf, true));  // row_shr:1
    v = add_ref(v, VRT_DPP_ZERO(v, 0x112, 0xf, true));  // row_shr:2
    v = add_ref(v, VRT_DPP_ZERO(v, 0x114, 0xf, true));  // row_shr:4
    v = add_ref(v, VRT_DPP_ZERO(v, 0x118, 0xf, true));  // row_shr:8
    v = add_ref(v, VRT_DPP_ZERO(v, 0x142, 0xa, false)); // row_bcast:15 into rows 1 and 3
    v = add_ref(v, VRT_DPP_ZERO(v, 0x143, 0xc, false)); // row_bcast:31 into rows 2 and 3
    return lane_value(v, 63);
}

// The kernel arguments reach the functions below through POINTERS (Pp, Sp), not references: a reference parameter promises the compiler
// that the whole structure may be read ahead of the branches that guard a read, and it then lifts the argument loads out of the loops --
// other machine code than the kernels had with this text in their bodies, with more registers live (one instantiation lost a wave per SIMD).
// ---------------------------------------------------------------------------------------------
// lane = ray (ray_short_kernel, ray_short_trans_kernel, ray_short_depth_kernel)
// ---------------------------------------------------------------------------------------------
// What the cull of one lane counted for the statistics
struct RayCullCounts { uint32_t chunks_kept, members, groups_kept, leaf_tests; };

// The cull of the lane = ray kernels: chunk spheres per lane, members of the chunks some lane keeps with a wave-uniform index.  Files
// the lane's list into s_list[k*64 + lane] (RAY_PL entries per lane: consecutive lanes on consecutive banks) in ascending scene order
// and returns its length, which runs on past RAY_PL: such a ray's list is not used.
template <int SRC>
__device__ __forceinline__ uint32_t ray_short_cull(const RayArgs *Pp, const SceneTables *Sp, uint32_t N, uint32_t nch /* (N + 63) / 64 */, uint32_t *s_list,
                                                   uint32_t lane, bool valid, const LaneRay &ray, RayCullCounts &cnt)
{
    const RayArgs &P = *Pp;
    const SceneTables &S = *Sp;
    uint32_t nl = 0, chunks_kept = 0, members = 0;
    [[maybe_unused]] uint32_t groups_kept = 0, leaf_tests = 0;
    if constexpr (SRC == RAY_LIST_INDEX) {
        // ---- the same cull through the Morton index: group spheres, the leaf spheres of the groups some lane keeps, the members of the
        // leaves some lane keeps -- all three with a wave-uniform index (scalar loads of consecutive permuted rows).  The leaf spheres
        // take the place of the chunk spheres (nch of them, 64 consecutive Morton positions each).
        const uint32_t ngr = (nch + 63u) / 64u;
        for (uint32_t g = 0; g < ngr; ++g) {
            const bool kg = valid && ray_chunk_keeps(uload(P.groups, g), ray);
            if (__ballot(kg) == 0ull) continue;
            groups_kept += kg ? 1u : 0u;
            const uint32_t lf0 = g * 64u, lf1 = min(lf0 + 64u, nch);
            leaf_tests += lf1 - lf0;
            for (uint32_t lf = lf0; lf < lf1; ++lf) {
                // a lane files only what its OWN group and leaf tests admit
                const bool kc = kg && ray_chunk_keeps(uload(P.leaves, lf), ray);
                if (__ballot(kc) == 0ull) continue;
                chunks_kept += kc ? 1u : 0u;
                const uint32_t first = lf * 64u, last = min(first + 64u, N);
                members += last - first;
#pragma unroll 2
                for (uint32_t pos = first; pos < last; ++pos) {
                    const bool km = ray_member_keeps(uload(P.mu_sig_m, pos), uload(P.gB_m, pos), ray);
                    if (kc && km) {
                        if (nl < (uint32_t)RAY_PL) {
                            // entries arrive in Morton order: filed at their place in ascending SCENE order, the order the shading sums in
                            const uint32_t idx = uload_u32(P.perm, pos);
                            uint32_t k = nl;
                            while (k > 0u) {
                                const uint32_t prev = s_list[(k - 1u) * 64u + lane];
                                if (prev < idx) break;
                                s_list[k * 64u + lane] = prev;
                                --k;
                            }
                            s_list[k * 64u + lane] = idx;
                        }
                        ++nl; // the count runs on: such a ray's list is not used
                    }
                }
            }
        }
    } else
    for (uint32_t c = 0; c < nch; ++c) {
        const bool kc = valid && ray_chunk_keeps(uload(P.chunks, c), ray);
        if (__ballot(kc) == 0ull) continue;
        chunks_kept += kc ? 1u : 0u;
        const uint32_t first = c * 64u, last = min(first + 64u, N);
        members += last - first;
#pragma unroll 4
        for (uint32_t idx = first; idx < last; ++idx) {
            // a lane files only what its OWN chunk test admits: its list does not depend on its wave-mates
            const bool km = ray_member_keeps(uload(S.mu_sig, idx), uload(S.gB, idx), ray);
            if (kc && km) {
                if (nl < (uint32_t)RAY_PL) s_list[nl * 64u + lane] = idx; // ascending; the count runs on
                ++nl;
            }
        }
    }
    cnt.chunks_kept = chunks_kept; cnt.members = members; cnt.groups_kept = groups_kept; cnt.leaf_tests = leaf_tests;
    return nl;
}

// Behind the cull: a ray whose list outgrew RAY_PL goes to the one-wave-per-ray kernel behind this one; the statistics of the lane.
template <int SRC>
__device__ __forceinline__ void ray_short_file(const RayArgs *Pp, uint32_t nch, uint64_t r, bool valid, bool is_long, uint32_t nl, const RayCullCounts &cnt)
{
    const RayArgs &P = *Pp;
    if (is_long) {
        const uint32_t pos = atomicAdd(&P.counters[0], 1u);
        if (pos < P.queue_cap) P.queue[pos] = (uint32_t)r;
    }
    if (P.stats && valid) {
        atomicAdd(&P.stats[0], 1ull);
        atomicAdd(&P.stats[is_long ? 2 : 1], 1ull);
        if (!is_long) { atomicAdd(&P.stats[3], (unsigned long long)nl); atomicAdd(&P.stats[4], (unsigned long long)nl * nl); }
        if constexpr (SRC == RAY_LIST_INDEX) {
            atomicAdd(&P.index_stats[0], (unsigned long long)((nch + 63u) / 64u));
            atomicAdd(&P.index_stats[1], (unsigned long long)cnt.groups_kept);
            atomicAdd(&P.index_stats[2], (unsigned long long)cnt.leaf_tests);
            atomicAdd(&P.index_stats[3], (unsigned long long)cnt.chunks_kept);
            atomicAdd(&P.index_stats[4], (unsigned long long)cnt.members);
        } else {
            atomicAdd(&P.stats[5], (unsigned long long)nch);
            atomicAdd(&P.stats[6], (unsigned long long)cnt.chunks_kept);
            atomicAdd(&P.stats[7], (unsigned long long)cnt.members);
        }
    }
}

// The statistics of a lane whose list came from a ray plan: the per-ray words ray_short_file counts, and none of the tests.
__device__ __forceinline__ void ray_plan_short_stats(const RayArgs *Pp, bool valid, bool is_long, uint32_t nl)
{
    const RayArgs &P = *Pp;
    if (P.stats && valid) {
        atomicAdd(&P.stats[0], 1ull);
        atomicAdd(&P.stats[is_long ? 2 : 1], 1ull);
        if (!is_long) { atomicAdd(&P.stats[3], (unsigned long long)nl); atomicAdd(&P.stats[4], (unsigned long long)nl * nl); }
    }
}

// A lane's ray behind its cull, as every lane = ray kernel begins: the ray (a lane past the end of the bundle works on the ray of the
// last slot and writes nothing), its list in s_list[k*64 + lane], filed to the long-ray queue and counted.
struct ShortRay {
    uint64_t r, rc;  // the lane's ray id, and the same clamped to the bundle
    bool valid, is_long, writes /* valid && !is_long: this lane's result is this kernel's to store */;
    uint32_t nl;     // list length; 0 for a long ray, whose list is not used here
    uint32_t nmax;   // the longest nl of the wave: its loops run that far, so that the wave stays together
    LaneRay ray;
};
// Which ray a lane of a lane = ray kernel works on: slot 64 * workgroup + lane of the bundle's own order, or of the sorted order
// (P.order: vrt_hip_set_ray_sort).  Everything behind this addresses rays, results, the queue and the records by the ray id.
struct ShortSlot { uint64_t r, rc; bool valid; }; // ShortRay's fields of these names
__device__ __forceinline__ ShortSlot ray_short_slot(const RayArgs *Pp, uint32_t lane)
{
    const RayArgs &P = *Pp;
    ShortSlot s;
    const uint64_t slot = (uint64_t)blockIdx.x * 64u + lane;
    s.valid = slot < P.nrays; // the grid has no wave without a valid ray
    s.rc = s.valid ? slot : P.nrays - 1;
    if (P.order) s.rc = P.order[s.rc];
    s.r = s.valid ? s.rc : slot;
    return s;
}
template <int SRC>
__device__ __forceinline__ ShortRay ray_short_begin(const RayArgs *Pp, const SceneTables *Sp, uint32_t *s_list /*[RAY_PL * 64]*/, uint32_t lane)
{
    const RayArgs &P = *Pp;
    ShortRay R;
    const ShortSlot s = ray_short_slot(Pp, lane);
    R.r = s.r; R.rc = s.rc; R.valid = s.valid;
    R.ray = load_ray(P, R.rc);
    if constexpr (SRC == RAY_LIST_PLAN) {
        // ---- the list of a ray plan: no sphere test, no member test, and the queue of the long rays is the plan's, made with it ----
        R.nl = R.valid ? P.pl_len[R.rc] : 0u;
        R.is_long = R.nl > (uint32_t)RAY_PL;
        if (!R.is_long) {
            const uint32_t *mine = P.pl_entries + P.pl_off[R.rc];
            for (uint32_t k = 0; k < R.nl; ++k) s_list[k * 64u + lane] = mine[k];
        }
        ray_plan_short_stats(Pp, R.valid, R.is_long, R.nl);
    } else {
        const uint32_t N = Sp->n, nch = (N + 63u) / 64u;
        RayCullCounts cnt;
        R.nl = ray_short_cull<SRC>(Pp, Sp, N, nch, s_list, lane, R.valid, R.ray, cnt);
        R.is_long = R.nl > (uint32_t)RAY_PL;
        ray_short_file<SRC>(Pp, nch, R.r, R.valid, R.is_long, R.nl, cnt); // to the one-wave-per-ray kernel behind this one; statistics
    }
    if (R.is_long) R.nl = 0;
    R.nmax = wave_max_u32(R.nl);
    R.writes = R.valid && !R.is_long;
    return R;
}

// ---------------------------------------------------------------------------------------------
// one wave per ray (ray_long_kernel, ray_long_trans_kernel, ray_long_depth_kernel)
// ---------------------------------------------------------------------------------------------
// The next entry of the long-ray queue for this wave.
// Every lane executes the atomic (lane 0 adds 1, the others 0: one wave-level atomic after the compiler's atomic optimizer).
// With `if (lane == 0) k = atomicAdd(..)` the compiler threaded lane 0's store at the end of the loop body into this claim and
// left the other 63 lanes in a loop of their own, reading k = 0 for ever: a claim must not sit behind a branch on the lane.
__device__ __forceinline__ uint32_t ray_long_claim(const RayArgs *Pp, uint32_t lane)
{
    const RayArgs &P = *Pp;
    return __builtin_amdgcn_readfirstlane(atomicAdd(&P.counters[1], lane == 0 ? 1u : 0u));
}

// The re-cull of one queued ray by its wave: 64 chunk spheres at a time (lane = chunk), then the members of the kept ones (lane =
// Gaussian).  The ray is wave-uniform: its survivors are compacted in index order (ballot / mbcnt, as the block cull does) into
// s_list[RAY_LCAP], and beyond RAY_LCAP into this workgroup's scratch slot of N words (entry k at slot[k]), so no list length is refused.
// INDEXED: the re-cull goes through the Morton index (lane = group, lane = leaf of a kept group, lane = member of a kept leaf) and finds
// the survivors in Morton order; each sets bit perm[pos] of this workgroup's bitmap (N bits of device memory, all zero between rays),
// and the list is read off the bitmap in ascending scene order -- the list the unindexed compaction makes.
// Returns the list length; ray_long_next's barriers stand before (the previous ray's list reads are done) and behind it.
template <int SRC>
__device__ __forceinline__ uint32_t ray_long_cull(const RayArgs *Pp, const SceneTables *Sp, uint32_t N, uint32_t nch /* (N + 63) / 64 */, lds_u32 *s_list,
                                                  uint32_t *slot, uint32_t lane, const LaneRay &ray)
{
    const RayArgs &P = *Pp;
    const SceneTables &S = *Sp;
    uint32_t n = 0;
    if constexpr (SRC == RAY_LIST_INDEX) {
        const uint32_t ngr = (nch + 63u) / 64u, nwords = (N + 31u) / 32u;
        uint32_t *bm = P.bitmap + (size_t)blockIdx.x * nwords;
        for (uint32_t g0 = 0; g0 < ngr; g0 += 64u) {
            const uint32_t g = g0 + lane;
            unsigned long long gmask = __ballot(g < ngr && ray_chunk_keeps(P.groups[min(g, ngr - 1u)], ray));
            while (gmask) {
                const uint32_t lf0 = (g0 + (uint32_t)__builtin_ctzll(gmask)) * 64u, lf = lf0 + lane;
                gmask &= gmask - 1ull;
                unsigned long long cmask = __ballot(lf < nch && ray_chunk_keeps(P.leaves[min(lf, nch - 1u)], ray));
                while (cmask) {
                    const uint32_t pos = (lf0 + (uint32_t)__builtin_ctzll(cmask)) * 64u + lane;
                    cmask &= cmask - 1ull;
                    const uint32_t pc = min(pos, N - 1u);
                    if (pos < N && ray_member_keeps(P.mu_sig_m[pc], P.gB_m[pc], ray)) {
                        const uint32_t idx = P.perm[pc];
                        if (idx < N) atomicOr(&bm[idx >> 5], 1u << (idx & 31u)); // lanes may share a word
                    }
                }
            }
        }
        __threadfence(); // the bits are in memory before they are taken out again
        // lane = word: take the word and leave zero behind (an atomic: the value in memory, whatever this CU's cache holds of the
        // last ray), then every lane files its bits from the wave's running count on -- ascending scene index
        for (uint32_t w0 = 0; w0 < nwords; w0 += 64u) {
            const uint32_t w = w0 + lane;
            uint32_t bits = w < nwords ? atomicExch(&bm[w], 0u) : 0u;
            const uint32_t cnt = (uint32_t)__popc(bits), incl = wave_inclusive_sum(cnt);
            uint32_t pos = n + incl - cnt;
            while (bits) {
                const uint32_t idx = w * 32u + (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1u;
                if (pos < (uint32_t)RAY_LCAP) s_list[pos] = idx;
                else if (pos < N) slot[pos] = idx;
                ++pos;
            }
            n += lane_value_u32(incl, 63u);
        }
    } else
    for (uint32_t c0 = 0; c0 < nch; c0 += 64u) {
        const uint32_t c = c0 + lane;
        unsigned long long cmask = __ballot(c < nch && ray_chunk_keeps(P.chunks[min(c, nch - 1u)], ray));
        while (cmask) {
            const uint32_t idx = (c0 + (uint32_t)__builtin_ctzll(cmask)) * 64u + lane;
            cmask &= cmask - 1ull;
            const uint32_t ic = min(idx, N - 1u);
            const bool keep = idx < N && ray_member_keeps(S.mu_sig[ic], S.gB[ic], ray);
            const unsigned long long mask = __ballot(keep);
            const uint32_t pos = n + lane_rank(mask);
            if (keep) {
                if (pos < (uint32_t)RAY_LCAP) s_list[pos] = idx;
                else if (pos < N) slot[pos] = idx;
            }
            n += (uint32_t)__popcll(mask);
        }
    }
    return min(n, N);
}

// entry p of a long ray's list: the first RAY_LCAP in LDS, the rest in the workgroup's scratch slot
__device__ __forceinline__ uint32_t long_list_entry(const uint32_t *s_list, const uint32_t *slot, uint32_t p)
{
    return p < (uint32_t)RAY_LCAP ? s_list[p] : slot[p];
}

// A wave's way through the long-ray queue, as every one-wave-per-ray kernel runs it:
//     LongRay L = ray_long_begin<SRC>(&P);
//     while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) { ... L.r, L.ray, the L.n entries long_list_entry(s_list, L.slot, p) ... }
struct LongRay {
    uint32_t n_long; // length of the queue
    uint32_t *slot;  // this workgroup's scratch slot; RAY_LIST_PLAN: the claimed ray's list in the plan (entry p at slot[p], as in a slot)
    uint32_t N, nch; // Gaussians and chunks of the scene
    uint64_t r;      // the ray claimed last,
    LaneRay ray;
    uint32_t n;      // and the length of its list
};
template <int SRC>
__device__ __forceinline__ LongRay ray_long_begin(const RayArgs *Pp)
{
    const RayArgs &P = *Pp;
    LongRay L;
    if constexpr (SRC == RAY_LIST_PLAN) {
        L.n_long = P.pl_nlong; // the plan's queue: nothing was filed by the short kernel
        L.slot = nullptr;
    } else {
        L.n_long = min(P.counters[0], P.queue_cap); // final: the short kernel is done
        L.slot = P.scratch + (size_t)blockIdx.x * P.S.n;
    }
    L.N = P.S.n; L.nch = (L.N + 63u) / 64u;
    return L;
}
// Claims the next ray of the queue and culls it again into s_list[RAY_LCAP] / L.slot; false when the queue is empty.  The whole wave
// calls this (ray_long_claim says why the claim sits behind no branch on the lane) and comes back together.
// RAY_LIST_PLAN: the queue and the list are the plan's -- the first RAY_LCAP entries copied to s_list, L.slot pointed at the list, so that
// long_list_entry reads the rest where it stands.  The work counter is still the context's.
// (ray_long_kernel of vrt_ray_kernel.hip runs a text of its own of this loop; the note at the top of that file says why.)
template <int SRC>
__device__ __forceinline__ bool ray_long_next(const RayArgs *Pp, const SceneTables *Sp, uint32_t *s_list /*[RAY_LCAP]*/, uint32_t lane, LongRay &L)
{
    const RayArgs &P = *Pp;
    while (true) {
        const uint32_t k = ray_long_claim(Pp, lane);
        if (k >= L.n_long) return false;
        if constexpr (SRC == RAY_LIST_PLAN) L.r = P.pl_long[k];
        else L.r = P.queue[k];
        if (L.r >= P.nrays) continue;
        L.ray = load_ray(P, L.r);
        __syncthreads(); // the previous ray's list reads are done
        if constexpr (SRC == RAY_LIST_PLAN) {
            L.slot = const_cast<uint32_t *>(P.pl_entries + P.pl_off[L.r]);
            L.n = min(P.pl_len[L.r], L.N);
            for (uint32_t p = lane; p < min(L.n, (uint32_t)RAY_LCAP); p += 64u) s_list[p] = L.slot[p];
        } else L.n = ray_long_cull<SRC>(Pp, Sp, L.N, L.nch, (lds_u32 *)s_list, L.slot, lane, L.ray);
        __syncthreads(); // list and scratch writes of this wave are visible to it
        if (P.stats && lane == 0 && L.n > (uint32_t)RAY_LCAP) atomicAdd(&P.stats[8], 1ull);
        return true;
    }
}

// Both kernels of a bundle, always enqueued: lane = ray over all rays, then one wave per queued ray on long_grid workgroups.
typedef void (*RayKernel)(RayArgs);
inline void launch_ray_kernels(RayKernel short_kernel, RayKernel long_kernel, const RayArgs &a, uint32_t long_grid, hipStream_t st)
{
    hipLaunchKernelGGL(short_kernel, dim3((uint32_t)((a.nrays + 63u) / 64u)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(long_kernel, dim3(long_grid), dim3(64), 0, st, a);
}

} // namespace vrtk
