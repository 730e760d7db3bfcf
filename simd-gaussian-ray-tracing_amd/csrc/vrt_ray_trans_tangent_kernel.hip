// vrt_ray_trans_tangent_kernel.hip -- transmittance tangent bundles (vrt_hip_transmittance_bundle_tangent*): J . v of the transmittance
// at sample distances along caller-given rays, forward mode -- or, in depth mode, J . v of the depth at which T falls to a level, at the
// depths a depth bundle returned.  The direction: a row per Gaussian in the gradient table's layout (columns 4..8 are read: d mu xyz,
// d sigma, d magnitude), a row per ray in the ray rows' layout (d origin, d direction) and a float per sample (d s_k, or d tau_k in depth
// mode), each nullable.  The rays, the cull, the lists, the queue of the long rays, the re-cull and the statistics are vrt_ray_cull.hpp's:
// the same rays keep the same Gaussians and go to the same kind of kernel as in every other bundle.  The kept list K of a ray is held
// fixed, and the function is the transmittance gradient bundles' (vrt_ray_trans_grad_kernel.hip has it): this is their transpose, term
// for term.
//
// The derivative ("Transmittance tangent bundles"; C = 2 / sqrt(pi)); per (ray, kept Gaussian) tangent_gauss's three
// scalars dmubar_j, u_j (dA_j = (A_j / m_j) u_j, formed without m_j) and ds_j = dsigma_j / sigma_j:
//   dE_k = sum_j [ dA_j D_kj + A_j C e2_kj (dmubar_j r_j + x_kj ds_j) ] + F,     F = sum_j A_j C e1_j (m_j ds_j - dmubar_j r_j)   (once per ray)
//   wrt == VRT_HIP_TGRAD_T:      out[r, k] = T_k (dE_k + S_k ds_k)
//   wrt == VRT_HIP_TGRAD_DEPTH:  out[r, k] = (dtau_k / T_k - dE_k) / S_k    the implicit function theorem on T(depth, theta) = tau.  A sample
//       whose s_k is not finite or <= 0, or whose S_k == 0, gets exactly 0: it is carried at s = 0 and its result is a select.
//   ray_short_trans_tangent_kernel  lane = ray.  One walk of the lane's list leaves the three scalars per (list position, lane) in LDS
//                                   (grad_acc's layout, as ray_short_tangent_kernel: 24 KB next to the 8 KB of lists) and sums F; columns
//                                   4..11 of a tangent row are read there, once, as two 16-byte loads.  Then per group of RAY_SG samples ONE
//                                   walk (grad_walk_begin / _next) with E_k, S_k and dE_k side by side: 12 accumulators.
//   ray_long_trans_tangent_kernel   one wave per queued ray, lane l takes entries l, l + 64, ...  Per group of RAY_SG samples every lane
//                                   walks its entries; E_k, S_k and dE_k by three wave_sums per sample in the wave's fixed order, stored by
//                                   lane 0.  The samples are wave-uniform and read where they are used: no LDS stage, no chunks.  The three
//                                   scalars of an entry are formed again in every group (the list has no bound, so they have no place
//                                   to wait in; DESIGN.md has the cost).  F is summed in the first group's walk.
// Every result is a STORE by the lane that owns it: no atomic add, no table, bitwise reproducible.  A lane past the end of its list reads
// row 0 of the table and uses none of it (a select); a Gaussian the ray drops is never read.
// Exp / Erf of the forward quantities are the selected pair's; e1 and e2 are exp_neg_sq<EXP>.  Only the four pairs of
// VRT_DISPATCH_GRAD_PAIR are instantiated; the entry point refuses the others.  wrt is read at run time (wave-uniform), as the gradient
// kernels read it.  Compiled with the default scheduler, like them.
#include "vrt_ray_grad.hpp"
#include "vrt_ray_trans.hpp" // RAY_SG

namespace vrtk {

// One absorber q with the tangent scalars g against RAY_SG samples: its terms of E_k, S_k and dE_k (without F).  `on` = false: nothing moves.
template <int EXP, int ERF>
__device__ __forceinline__ void trans_tangent_pair(const ErfEval<ERF> &erf, const GradGauss &q, const TanGauss &g, bool on, const float (&sv)[RAY_SG],
                                                   float (&accE)[RAY_SG], float (&accS)[RAY_SG], float (&accD)[RAY_SG])
{
    const float AC = q.A * ERF_SLOPE;
    const float dA = q.Am * g.u;
    const float dmr = g.dmubar * q.r;
#pragma unroll
    for (int k = 0; k < RAY_SG; ++k) {
        const float x = trans_grad_x(sv[k], q);
        const float D = q.E - erf(x);
        const float e2 = exp_neg_sq<EXP>(x);
        const float e = __builtin_fmaf(q.A, D, accE[k]);
        const float t = __builtin_fmaf(-q.Ar, e2, accS[k]);
        const float d = __builtin_fmaf(dA, D, __builtin_fmaf(AC * e2, __builtin_fmaf(x, g.ds, dmr), accD[k]));
        accE[k] = on ? e : accE[k];
        accS[k] = on ? t : accS[k];
        accD[k] = on ? d : accD[k];
    }
}
// q's term of F, the part of dE_k that no sample moves
template <int EXP>
__device__ __forceinline__ float trans_tangent_F(const GradGauss &q, const TanGauss &g, bool on, float F)
{
    const float f = __builtin_fmaf((q.A * ERF_SLOPE) * exp_neg_sq<EXP>(q.m), __builtin_fmaf(q.m, g.ds, -(g.dmubar * q.r)), F);
    return on ? f : F;
}
// What leaves per sample once E_k, S_k and dE_k (F included) are known.  live: trans_grad_live of the sample (depth mode: s_k is finite and > 0; T mode: always).
template <int EXP>
__device__ __forceinline__ float trans_tangent_result(bool depth_mode, bool live, float E, float Sk, float dE, float sdot)
{
    const float T = vexp<EXP>(E);
    if (depth_mode) {
        const bool ok = live && Sk != 0.f;
        return ok ? (sdot / T - dE) / Sk : 0.f;
    }
    return T * __builtin_fmaf(Sk, sdot, dE);
}

template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_short_trans_tangent_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    __shared__ float s_tan[3 * RAY_PL * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane); // the cull: exactly the radiance kernel's
    const uint32_t nl = R.nl, nmax = R.nmax;
    const LaneRay &ray = R.ray;
    const LaneList L = { s_list, lane, nl, nmax };
    const ErfEval<ERF> erf;
    const TanRay tr = tangent_ray(P.ray_tangent, R.rc);
    const bool depth_mode = P.wrt == VRT_HIP_TGRAD_DEPTH;
    const uint64_t ns = P.ns;
    const float *sp = P.s + (P.s_per_ray ? R.rc * ns : 0ull);
    const float *tp = P.s_tangent ? P.s_tangent + (P.s_tangent_per_ray ? R.rc * ns : 0ull) : nullptr;
    float *op = P.trans_tangent_out + R.rc * ns;

    // ---- the tangent rows of the lane's list, each read once, to three scalars per position; and F ----
    float F = 0.f;
    {
        ListWalk lw = grad_walk_begin(S, L);
        for (uint32_t j = 0; j < nmax; ++j) {
            const uint32_t idx = L.at(j);
            const bool on = L.has(j);
            const GradGauss q = grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j);
            float4 ms_t = make_float4(0.f, 0.f, 0.f, 0.f);
            float dm = 0.f;
            if (P.tangent) tangent_row_load(P.tangent, idx, ms_t, dm); // wave-uniform
            const TanGauss g = tangent_gauss(q, ray, tr, on ? S.gD[idx].z : 0.f, ms_t, dm, on);
            grad_acc(s_tan, 0, j, lane) = g.dmubar;
            grad_acc(s_tan, 1, j, lane) = g.u;
            grad_acc(s_tan, 2, j, lane) = g.ds;
            F = trans_tangent_F<EXP>(q, g, on, F);
        }
    }

    for (uint64_t k0 = 0; k0 < ns; k0 += RAY_SG) {
        float sv[RAY_SG], dv[RAY_SG], accE[RAY_SG], accS[RAY_SG], accD[RAY_SG];
        bool live[RAY_SG];
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g) {
            const bool in = R.writes && k0 + g < ns;
            const float s = in ? sp[k0 + g] : 0.f;
            live[g] = trans_grad_live(depth_mode, s, 1.f);
            sv[g] = live[g] ? s : 0.f;
            dv[g] = in && tp ? tp[k0 + g] : 0.f;
            accE[g] = accS[g] = accD[g] = 0.f;
        }
        // ---- the one walk: E_k, S_k and dE_k ----
        ListWalk lw = grad_walk_begin(S, L);
        for (uint32_t j = 0; j < nmax; ++j) {
            const GradGauss q = grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j);
            const TanGauss g = { grad_acc(s_tan, 0, j, lane), grad_acc(s_tan, 1, j, lane), grad_acc(s_tan, 2, j, lane) };
            trans_tangent_pair<EXP>(erf, q, g, L.has(j), sv, accE, accS, accD);
        }
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g) {
            const float v = trans_tangent_result<EXP>(depth_mode, live[g], accE[g], accS[g], accD[g] + F, dv[g]);
            if (R.writes && k0 + g < ns) op[k0 + g] = v; // a ray that keeps nothing: exact zeros
        }
    }
}

// One wave per long ray, lane l takes entries l, l + 64, ...
template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_long_trans_tangent_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    const ErfEval<ERF> erf;
    const bool depth_mode = P.wrt == VRT_HIP_TGRAD_DEPTH;
    const uint64_t ns = P.ns;

    LongRay L = ray_long_begin<SRC>(&P);
    while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) {
        const LaneRay ray = L.ray;
        const uint32_t n = L.n;
        const TanRay tr = tangent_ray(P.ray_tangent, L.r);
        const float *sp = P.s + (P.s_per_ray ? L.r * ns : 0ull);
        const float *tp = P.s_tangent ? P.s_tangent + (P.s_tangent_per_ray ? L.r * ns : 0ull) : nullptr;
        float *op = P.trans_tangent_out + L.r * ns;
        float F = 0.f; // the wave's sum behind the first group
        for (uint64_t k0 = 0; k0 < ns; k0 += RAY_SG) {
            float sv[RAY_SG], dv[RAY_SG], accE[RAY_SG], accS[RAY_SG], accD[RAY_SG];
            bool live[RAY_SG];
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) { // wave-uniform
                const bool in = k0 + g < ns;
                const float s = in ? sp[k0 + g] : 0.f;
                live[g] = trans_grad_live(depth_mode, s, 1.f);
                sv[g] = live[g] ? s : 0.f;
                dv[g] = in && tp ? tp[k0 + g] : 0.f;
                accE[g] = accS[g] = accD[g] = 0.f;
            }
            float Fl = 0.f;
            for (uint32_t p = lane; p < n; p += 64u) {
                const uint32_t idx = long_list_entry(s_list, L.slot, p);
                const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], true, ray);
                float4 ms_t = make_float4(0.f, 0.f, 0.f, 0.f);
                float dm = 0.f;
                if (P.tangent) tangent_row_load(P.tangent, idx, ms_t, dm); // wave-uniform
                const TanGauss g = tangent_gauss(q, ray, tr, S.gD[idx].z, ms_t, dm, true);
                if (k0 == 0) Fl = trans_tangent_F<EXP>(q, g, true, Fl); // wave-uniform
                trans_tangent_pair<EXP>(erf, q, g, true, sv, accE, accS, accD);
            }
            if (k0 == 0) F = wave_sum(Fl); // the whole wave is here again
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) {
                const float E = wave_sum(accE[g]), Sk = wave_sum(accS[g]), dE = wave_sum(accD[g]);
                const float v = trans_tangent_result<EXP>(depth_mode, live[g], E, Sk, dE + F, dv[g]);
                if (lane == 0 && k0 + g < ns) op[k0 + g] = v;
            }
        }
    }
}

template <int EXP, int ERF>
static void launch_ray_trans_tangent_bundle_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    if (src == RAY_LIST_PLAN) launch_ray_kernels(ray_short_trans_tangent_kernel<EXP, ERF, RAY_LIST_PLAN>, ray_long_trans_tangent_kernel<EXP, ERF, RAY_LIST_PLAN>, a, long_grid, st);
    else if (src == RAY_LIST_INDEX) launch_ray_kernels(ray_short_trans_tangent_kernel<EXP, ERF, RAY_LIST_INDEX>, ray_long_trans_tangent_kernel<EXP, ERF, RAY_LIST_INDEX>, a, long_grid, st);
    else launch_ray_kernels(ray_short_trans_tangent_kernel<EXP, ERF, RAY_LIST_CHUNKS>, ray_long_trans_tangent_kernel<EXP, ERF, RAY_LIST_CHUNKS>, a, long_grid, st);
}
void launch_ray_trans_tangent_bundle(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !a.ns || !long_grid || !a.trans_tangent_out || !ray_grad_pair_supported(exp_kind, erf_kind)) return;
    VRT_DISPATCH_GRAD_PAIR(launch_ray_trans_tangent_bundle_t, a, long_grid, src, st);
}

} // namespace vrtk
