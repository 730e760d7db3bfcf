// vrt_ray_grad.hpp -- what the derivative kernels of the ray bundles share: vrt_ray_grad_kernel.hip (d radiance / d Gaussians) and
// vrt_ray_trans_grad_kernel.hip (d transmittance / d Gaussians and samples, d depth / d Gaussians and levels).  One Gaussian against
// one ray with the compensated c = mu - o and mubar = c . n that keep d / d mu accurate (grad_gauss), and the deposit of a row segment
// into the caller's table, wave-summed where every lane names the same row (grad_deposit).  One text for both translation units: the
// same (ray, Gaussian) gives the same A, c_perp, d2 and Erf(-mubar r) in either kind of gradient.
#pragma once
#include "vrt_ray_cull.hpp"

namespace vrtk {

constexpr float ERF_SLOPE = 1.1283791670955126f; // 2 / sqrt(pi): Erf'(x) = ERF_SLOPE exp(-x^2)
constexpr int GRAD_STRIDE = VRT_HIP_GRAD_STRIDE; // floats per row of the caller's table

// a - b as an unevaluated sum hi + lo, exactly (Knuth's two-sum on a and -b)
__device__ __forceinline__ void exact_diff(float a, float b, float &hi, float &lo)
{
    hi = sub_ref(a, b);
    const float bb = sub_ref(hi, a);
    lo = sub_ref(sub_ref(a, sub_ref(hi, bb)), add_ref(b, bb));
}

// One Gaussian against one ray, as both passes and the last walk need it.  d2 is formed from c_perp = c - mubar n itself, not as
// |c|^2 - mubar^2: the vector is needed anyway and its norm has no cancellation.  c = mu - o keeps the low part its rounding drops: the
// exponent d2 / (2 sigma^2) of a small Gaussian far from the origin otherwise carries ulp(|c|) |c_perp| / sigma^2 of error, 1e-4 of a
// row's every entry in the grid scene seen from four units away (a rounding error of mubar only moves c_perp along n: second order).  `on` = false (a lane past the end of its list):
// a harmless row takes the place of whatever was loaded, and the weights are exact zeros.
struct GradGauss {
    float mubar, d2, px, py, pz; // c . n, |c_perp|^2, c_perp
    float r, inv_s, inv_s2;      // 1 / (sqrt2 sigma), 1 / sigma, 1 / sigma^2
    float A, Am, Ar;             // A_j, A_j / m_j (formed without m_j), A_j C r_j
    float m, E;                  // mubar r, Erf(-mubar r)
};
template <int EXP, int ERF>
__device__ __forceinline__ GradGauss grad_gauss(const ErfEval<ERF> &erf, float4 ms, float4 b, bool on, const LaneRay &ray)
{
    if (!on) { ms = make_float4(ray.ox, ray.oy, ray.oz, 1.f); b = make_float4(0.70710678f, 0.5f, 0.f, 0.f); }
    GradGauss q;
    float cx, cy, cz, lx, ly, lz;
    exact_diff(ms.x, ray.ox, cx, lx); exact_diff(ms.y, ray.oy, cy, ly); exact_diff(ms.z, ray.oz, cz, lz);
    // mubar = c . n as hi + lo (products split by fma, sums by two-sum, the low part of c included): a rounding error of mubar moves
    // c_perp along n -- second order in d2, but first order in a component of c_perp that is small against |c| |n's component|
    const float p1 = mul_ref(cx, ray.nx), p2 = mul_ref(cy, ray.ny), p3 = mul_ref(cz, ray.nz);
    const float e1 = __builtin_fmaf(cx, ray.nx, -p1), e2 = __builtin_fmaf(cy, ray.ny, -p2), e3 = __builtin_fmaf(cz, ray.nz, -p3);
    float s12, r12, s123, r123;
    exact_diff(p1, -p2, s12, r12);
    exact_diff(s12, -p3, s123, r123);
    const float tail = add_ref(add_ref(add_ref(add_ref(e1, e2), e3), add_ref(r12, r123)), dot3_ref(lx, ly, lz, ray.nx, ray.ny, ray.nz));
    q.mubar = add_ref(s123, tail);
    const float mlo = add_ref(sub_ref(s123, q.mubar), tail);
    q.px = add_ref(__builtin_fmaf(-mlo, ray.nx, __builtin_fmaf(-q.mubar, ray.nx, cx)), lx);
    q.py = add_ref(__builtin_fmaf(-mlo, ray.ny, __builtin_fmaf(-q.mubar, ray.ny, cy)), ly);
    q.pz = add_ref(__builtin_fmaf(-mlo, ray.nz, __builtin_fmaf(-q.mubar, ray.nz, cz)), lz);
    q.d2 = dot3_ref(q.px, q.py, q.pz, q.px, q.py, q.pz);
    const float ex = vexp<EXP>(-(q.d2 * b.y));
    q.r = b.x; q.inv_s = b.x * SQRT_2; q.inv_s2 = 2.f * b.y;
    q.A = b.z * ex;
    q.Am = on ? (INV_SQRT_2_PI * ms.w) * ex : 0.f;
    q.Ar = q.A * ERF_SLOPE * b.x;
    q.m = q.mubar * b.x;
    q.E = erf(-q.m);
    return q;
}

// NV values per lane for columns col0.. of row idx of the caller's table; `on`: this lane has something to add.  The whole wave calls
// this.  When every lane that is on names the same row, the values are summed over the wave and lanes 0..NV-1 add one segment.
template <int NV>
__device__ __forceinline__ void grad_deposit(float *table, uint32_t idx, bool on, const float (&v)[NV], uint32_t col0, uint32_t lane)
{
    const unsigned long long mask = __ballot(on);
    if (mask == 0ull) return;
    const uint32_t first = lane_value_u32(idx, (uint32_t)__builtin_ctzll(mask));
    const bool shared = __ballot(on && idx == first) == mask && (mask & (mask - 1ull)) != 0ull; // one row, more than one adder
    if (shared) {
        float mine = 0.f;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const float s = wave_sum(on ? v[c] : 0.f);
            if (lane == (uint32_t)c) mine = s;
        }
        if (lane < (uint32_t)NV) atomicAdd(&table[(size_t)first * GRAD_STRIDE + col0 + lane], mine);
    } else if (on) {
#pragma unroll
        for (int c = 0; c < NV; ++c) atomicAdd(&table[(size_t)idx * GRAD_STRIDE + col0 + c], v[c]);
    }
}

} // namespace vrtk
