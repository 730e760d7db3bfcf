// vrt_ray_trans.hpp -- the transmittance exponent along one ray, shared by vrt_ray_trans_kernel.hip (T at given depths) and
// vrt_ray_depth_kernel.hip (the depth at which T falls to a given level): a Gaussian's term cut into what depends on (ray, Gaussian)
// alone and what a sample distance adds to it, the number of samples carried through one walk of a list, and the entry of a long ray's
// list.  One text for both translation units: the two kinds of bundle evaluate the same function T(s) of a ray, bit for bit.
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

// entry p of a long ray's list: the first RAY_LCAP in LDS, the rest in the workgroup's scratch slot
__device__ __forceinline__ uint32_t long_list_entry(const uint32_t *s_list, const uint32_t *slot, uint32_t p)
{
    return p < (uint32_t)RAY_LCAP ? s_list[p] : slot[p];
}

} // namespace vrtk
