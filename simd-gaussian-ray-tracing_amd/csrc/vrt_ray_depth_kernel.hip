// vrt_ray_depth_kernel.hip -- depth bundles (vrt_hip_depth_bundle*): the distance along caller-given rays at which the transmittance
// falls to each of nt levels -- the inverse of the transmittance bundles' T(s) (vrt_ray_trans_kernel.hip), which is evaluated here by
// the walks those kernels call (short_walk, long_walk of vrt_ray_trans.hpp): the same text over the same lists in the same order, so
// that T(depth) through a transmittance bundle is the very number this search compared with the level.  The cull, the queue of the long rays, the re-cull and the statistics are
// vrt_ray_cull.hpp's: the same rays keep the same Gaussians and go to the same kind of kernel as in the other two bundles.
//   ray_short_depth_kernel  lane = ray, per-ray lists of at most RAY_PL scene indices in LDS; every lane searches its own brackets
//   ray_long_depth_kernel   one wave per ray whose list is longer; lane l takes entries l, l + 64, ..., wave_sum reduces the partial sums
//                           as ray_long_trans_kernel does; the brackets are wave-uniform, lane 0 stores
// The search (depth_bracket, depth_next below) is plain bisection in T-space: per ray one walk of the list for s_end and T(0), one for T(s_end),
// then per group of RAY_SG levels one walk per halving of the brackets [0, s_end] -- RAY_SG brackets ride on one walk -- until every
// bracket is no wider than max(ulp(hi), s_end 2^-24): 23 to 25 halvings.  An entry's (w, Erf(-mubar_n), mubar_n, sqrt2 sigma) are
// recomputed on every walk, not stashed: RAY_PL * 64 rows of 16 B would be 32 KB of LDS per wave.
// Compiled with the default scheduler, as the transmittance bundles are.
#include "vrt_ray_trans.hpp"

namespace vrtk {

constexpr int DEPTH_MAX_WALKS = 64; // of one group's search: never reached by a finite s_end (a bracket halves per walk)

// The brackets of one group of levels before its search.  A level that needs no search gets lo == hi == its result (NaN for a NaN level,
// 0 where T(0) <= tau, +inf where T(s_end) > tau -- a miss -- and 0 for a slot past the last level); the others [0, s_end], both ends evaluated.
__device__ __forceinline__ void depth_bracket(float tau, bool used, float T0, float Tend, float s_end, float &lo, float &hi)
{
    float v = s_end;
    bool search = used;
    if (!used) v = 0.f;
    else if (tau != tau) { v = tau; search = false; }
    else if (T0 <= tau) { v = 0.f; search = false; }
    else if (Tend > tau) { v = __builtin_inff(); search = false; }
    hi = v;
    lo = search ? 0.f : v;
}
// The next evaluation point of a bracket, or none: the bracket is as narrow as the contract asks (hi - lo <= max(ulp(hi), res): between
// neighbouring floats the midpoint is one of them), or it never was one (lo == hi, +inf, NaN).
__device__ __forceinline__ bool depth_next(float lo, float hi, float res, float &mid)
{
    mid = add_ref(lo, mul_ref(0.5f, sub_ref(hi, lo)));
    return sub_ref(hi, lo) > res && mid > lo && mid < hi;
}

template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_short_depth_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    const uint32_t lane = threadIdx.x & 63u;
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane); // the cull: exactly the radiance kernel's
    const uint32_t nl = R.nl, nmax = R.nmax;
    const LaneRay &ray = R.ray;

    // ---- the ends: s_end with T(0), then T(s_end); an empty list has s_end = 0 and T = Exp(0) at both ----
    float s1[1] = { 0.f }, e1[1];
    const float s_end = short_walk<EXP, ERF, 1, true>(&S, s_list, lane, nl, nmax, ray, s1, e1);
    const float T0 = vexp<EXP>(e1[0]);
    s1[0] = s_end;
    short_walk<EXP, ERF, 1, false>(&S, s_list, lane, nl, nmax, ray, s1, e1);
    const float Tend = vexp<EXP>(e1[0]);
    const float res = mul_ref(s_end, 0x1p-24f);

    // ---- levels, RAY_SG at a time: every walk of the lane's list halves the brackets of the whole group ----
    const uint64_t nt = P.nt;
    const float *tp = P.tau + (P.tau_per_ray ? R.rc * nt : 0ull);
    float *dp = P.depth + R.rc * nt;
    const bool writes = R.writes;
    for (uint64_t k0 = 0; k0 < nt; k0 += RAY_SG) {
        float tau[RAY_SG], lo[RAY_SG], hi[RAY_SG];
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g) {
            const bool used = k0 + g < nt;
            tau[g] = used ? tp[k0 + g] : 0.f;
            depth_bracket(tau[g], used && writes, T0, Tend, s_end, lo[g], hi[g]);
        }
        for (int it = 0; it < DEPTH_MAX_WALKS; ++it) {
            float sv[RAY_SG], acc[RAY_SG];
            bool act[RAY_SG], any = false;
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) {
                act[g] = depth_next(lo[g], hi[g], res, sv[g]);
                any = any || act[g];
                if (!act[g]) sv[g] = 0.f;
            }
            if (__ballot(any) == 0ull) break; // the loops below run to the wave's longest list: the wave stays together
            short_walk<EXP, ERF, RAY_SG, false>(&S, s_list, lane, nl, nmax, ray, sv, acc);
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) {
                const bool below = vexp<EXP>(acc[g]) <= tau[g];
                hi[g] = act[g] && below ? sv[g] : hi[g];
                lo[g] = act[g] && !below ? sv[g] : lo[g];
            }
        }
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g)
            if (writes && k0 + g < nt) dp[k0 + g] = hi[g];
    }
}

// One wave per long ray.  Claim, re-cull and list are the radiance long kernel's (vrt_ray_cull.hpp); everything below the list is
// wave-uniform: the wave's sums come back from wave_sum as scalars, so every lane holds the same brackets.
template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_long_depth_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nt = P.nt;

    LongRay L = ray_long_begin<SRC>(&P);
    while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) {
        const uint32_t *slot = L.slot;
        const uint32_t n = L.n;
        const LaneRay &ray = L.ray;

        float s1[1] = { 0.f }, e1[1];
        const float s_end = long_walk<EXP, ERF, 1, true>(&S, s_list, slot, lane, n, ray, s1, e1);
        const float T0 = vexp<EXP>(e1[0]);
        s1[0] = s_end;
        long_walk<EXP, ERF, 1, false>(&S, s_list, slot, lane, n, ray, s1, e1);
        const float Tend = vexp<EXP>(e1[0]);
        const float res = mul_ref(s_end, 0x1p-24f);

        const float *tp = P.tau + (P.tau_per_ray ? L.r * nt : 0ull);
        float *dp = P.depth + L.r * nt;
        for (uint64_t k0 = 0; k0 < nt; k0 += RAY_SG) {
            float tau[RAY_SG], lo[RAY_SG], hi[RAY_SG];
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) {
                const bool used = k0 + g < nt;
                tau[g] = used ? tp[k0 + g] : 0.f;
                depth_bracket(tau[g], used, T0, Tend, s_end, lo[g], hi[g]);
            }
            for (int it = 0; it < DEPTH_MAX_WALKS; ++it) {
                float sv[RAY_SG], total[RAY_SG];
                bool act[RAY_SG], any = false;
#pragma unroll
                for (int g = 0; g < RAY_SG; ++g) {
                    act[g] = depth_next(lo[g], hi[g], res, sv[g]);
                    any = any || act[g];
                    if (!act[g]) sv[g] = 0.f;
                }
                if (__ballot(any) == 0ull) break; // wave-uniform either way
                long_walk<EXP, ERF, RAY_SG, false>(&S, s_list, slot, lane, n, ray, sv, total);
#pragma unroll
                for (int g = 0; g < RAY_SG; ++g) {
                    const bool below = vexp<EXP>(total[g]) <= tau[g];
                    hi[g] = act[g] && below ? sv[g] : hi[g];
                    lo[g] = act[g] && !below ? sv[g] : lo[g];
                }
            }
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g)
                if (lane == 0 && k0 + g < nt) dp[k0 + g] = hi[g];
        }
    }
}

template <int EXP, int ERF>
static void launch_ray_depth_bundle_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    if (src == RAY_LIST_PLAN) launch_ray_kernels(ray_short_depth_kernel<EXP, ERF, RAY_LIST_PLAN>, ray_long_depth_kernel<EXP, ERF, RAY_LIST_PLAN>, a, long_grid, st);
    else if (src == RAY_LIST_INDEX) launch_ray_kernels(ray_short_depth_kernel<EXP, ERF, RAY_LIST_INDEX>, ray_long_depth_kernel<EXP, ERF, RAY_LIST_INDEX>, a, long_grid, st);
    else launch_ray_kernels(ray_short_depth_kernel<EXP, ERF, RAY_LIST_CHUNKS>, ray_long_depth_kernel<EXP, ERF, RAY_LIST_CHUNKS>, a, long_grid, st);
}
void launch_ray_depth_bundle(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !a.nt || !long_grid) return;
    VRT_DISPATCH_EXP_ERF(launch_ray_depth_bundle_t, a, long_grid, src, st);
}

} // namespace vrtk
