// vrt_ray_trans.hpp -- the transmittance exponent along one ray, shared by vrt_ray_trans_kernel.hip (T at given depths) and
// vrt_ray_depth_kernel.hip (the depth at which T falls to a given level): a Gaussian's term cut into what depends on (ray, Gaussian)
// alone and what a sample distance adds to it, the number of samples carried through one walk of a list, and the walk itself, of a
// lane's list (short_walk) and of a long ray's by its wave (long_walk).  One text for both translation units: the two kinds of bundle
// evaluate the same function T(s) of a ray over the same lists in the same order, bit for bit.
#pragma once
#include "vrt_ray_cull.hpp"

namespace vrtk {

// samples a lane (short kernel) or a wave (long kernel) carries through one walk of a list
constexpr int RAY_SG = 4;

// transmittance_term (vrt_kernels_common.hpp) cut in two: what depends on (ray, Gaussian) alone, and what a sample adds to it.  The same
// operations on the same operands in the same order -- nothing re-associated, nothing fused, exact divides.
struct TransEntry { float w /* sigma cbar / sqrt(2 pi) */, erf0 /* Erf(-mubar_n) */, mu_bar_n, sqrt_2_sig; };
template <int EXP, int ERF>
__device__ __forceinline__ TransEntry trans_entry(float4 g /* mu, sigma */, float mag, const LaneRay &ray)
{
    const float cx = sub_ref(g.x, ray.ox), cy = sub_ref(g.y, ray.oy), cz = sub_ref(g.z, ray.oz);
    const float mu_bar = dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz);
    const float oc_sq = dot3_ref(cx, cy, cz, cx, cy, cz);
    const float inv_2_sigma2 = 1.f / mul_ref(mul_ref(2.f, g.w), g.w);
    const float c_bar = mul_ref(mag, vexp<EXP>(-mul_ref(sub_ref(oc_sq, mul_ref(mu_bar, mu_bar)), inv_2_sigma2)));
    TransEntry t;
    t.sqrt_2_sig = mul_ref(SQRT_2, g.w);
    t.mu_bar_n = mu_bar / t.sqrt_2_sig;
    t.w = mul_ref(mul_ref(g.w, c_bar), INV_SQRT_2_PI);
    t.erf0 = verf<ERF>(-t.mu_bar_n);
    return t;
}
template <int ERF>
__device__ __forceinline__ float trans_sample(const TransEntry &t, float s)
{
    const float s_n = s / t.sqrt_2_sig;
    return mul_ref(t.w, sub_ref(t.erf0, verf<ERF>(sub_ref(s_n, t.mu_bar_n))));
}

// mu_bar + 6 sqrt(2) sigma of one Gaussian: beyond it every Erf of its term is saturated (Erf(6) rounds to 1); mu_bar in trans_entry's operations
__device__ __forceinline__ float trans_reach(float4 g /* mu, sigma */, const LaneRay &ray)
{
    const float cx = sub_ref(g.x, ray.ox), cy = sub_ref(g.y, ray.oy), cz = sub_ref(g.z, ray.oz);
    const float mu_bar = dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz);
    return add_ref(mu_bar, mul_ref(6.f, mul_ref(SQRT_2, g.w)));
}

// One walk of a lane's list (s_list[k*64 + lane], nl entries; the loop runs to nmax, the longest list of the wave's short rays, and a
// lane past the end of its list leaves its sums as they are): acc[g] = the exponent at sv[g], transmittance_term added in ascending
// scene order.  Returns, with REACH, the largest trans_reach of the list, at least 0 (without: 0).
template <int EXP, int ERF, int NS, bool REACH>
__device__ __forceinline__ float short_walk(const SceneTables *Sp, const uint32_t *s_list, uint32_t lane, uint32_t nl, uint32_t nmax, const LaneRay &ray,
                                            const float (&sv)[NS], float (&acc)[NS])
{
    const SceneTables &S = *Sp;
    float reach = 0.f;
#pragma unroll
    for (int g = 0; g < NS; ++g) acc[g] = 0.f;
    if (!nmax) return reach;
    uint32_t lj = nl ? s_list[lane] : 0u;
    float4 a = S.mu_sig[lj];
    float mag = S.gD[lj].z;
    for (uint32_t j = 0; j < nmax; ++j) {
        const float4 ca = a;
        const float cm = mag;
        const bool vj = j < nl;
        if (j + 1 < nmax) { // the next entry's rows, one iteration ahead
            lj = (j + 1 < nl) ? s_list[(j + 1) * 64 + lane] : 0u;
            a = S.mu_sig[lj]; mag = S.gD[lj].z;
        }
        const TransEntry t = trans_entry<EXP, ERF>(ca, cm, ray);
        if constexpr (REACH) reach = vj ? fmaxf(reach, trans_reach(ca, ray)) : reach;
#pragma unroll
        for (int g = 0; g < NS; ++g) {
            const float sum = add_ref(acc[g], trans_sample<ERF>(t, sv[g]));
            acc[g] = vj ? sum : acc[g];
        }
    }
    return reach;
}

// One walk of a long ray's list by its wave: lane l takes entries l, l + 64, ... with per-lane gathers of the rows; total[g] = the
// exponent at sv[g], the 64 partial sums reduced in a fixed order (wave_sum) -- wave-uniform, and another summation order than
// short_walk's.  The whole wave calls this.  Returns, with REACH, the largest trans_reach of the list, at least 0 (without: 0).
template <int EXP, int ERF, int NS, bool REACH>
__device__ __forceinline__ float long_walk(const SceneTables *Sp, const uint32_t *s_list, const uint32_t *slot, uint32_t lane, uint32_t n, const LaneRay &ray,
                                           const float (&sv)[NS], float (&total)[NS])
{
    const SceneTables &S = *Sp;
    float acc[NS], far = 0.f;
#pragma unroll
    for (int g = 0; g < NS; ++g) acc[g] = 0.f;
    for (uint32_t p = lane; p < n; p += 64u) {
        const uint32_t idx = long_list_entry(s_list, slot, p);
        const float4 ms = S.mu_sig[idx];
        const TransEntry t = trans_entry<EXP, ERF>(ms, S.gD[idx].z, ray);
        if constexpr (REACH) far = fmaxf(far, trans_reach(ms, ray));
#pragma unroll
        for (int g = 0; g < NS; ++g) acc[g] = add_ref(acc[g], trans_sample<ERF>(t, sv[g]));
    }
#pragma unroll
    for (int g = 0; g < NS; ++g) total[g] = wave_sum(acc[g]); // the whole wave is here again
    if constexpr (REACH) far = wave_max(far);
    return far;
}

} // namespace vrtk
