// vrt_ray_tangent_kernel.hip -- tangent bundles (vrt_hip_radiance_rays_tangent*): J . v of the radiance of caller-given rays, forward
// mode.  Given a direction in parameter space -- a row per Gaussian in the gradient table's layout (d albedo rgba, d mu xyz, d sigma,
// d magnitude) and a row per ray in the ray rows' layout (d origin, d direction) -- every ray gets the 4 floats by which its radiance
// moves along it.  The rays, the cull, the lists, the queue of the long rays, the re-cull and the statistics are vrt_ray_cull.hpp's, the
// text the radiance and the gradient kernels run: the same rays keep the same Gaussians and go to the same kind of kernel.  The kept
// list K of a ray is held fixed, as in the gradient bundles, and the function is theirs (vrt_ray_grad_kernel.hip has it).
//
// The derivative ("Tangent bundles"; C = 2 / sqrt(pi), dn the ray's direction tangent, of which c_perp . dn sees the part perpendicular to n):
//   dc_j = dmu_j - do,  cn_j = c_perp_j . dn,  dmubar_j = dc_j . n + cn_j,  dd2_j = 2 c_perp_j . dc_j - 2 mubar_j cn_j,  ds_j = dsigma_j / sigma_j
//   u_j = m_j (ds_j - dd2_j / (2 sigma_j^2) + d2_j ds_j / sigma_j^2) + dm_j            so that   dA_j = (A_j / m_j) u_j, formed without m_j
//   dx_ikj = (dmubar_i + k dsigma_i - dmubar_j) r_j - x_ikj ds_j
//   dacc_ik = sum_j [ dA_j D_ikj - A_j C e2_ikj dx_ikj ] + F,       F = sum_j A_j C e1_j (mubar_j r_j ds_j - dmubar_j r_j)   (the same for every i, k)
//   dL = sum_i [ da_i m_i V_i + a_i (u_i V_i + m_i sum_k t_ik dacc_ik) ],       t_ik the ik term of L without a_i m_i,  V_i = sum_k t_ik
// Three scalars per (ray, kept Gaussian) carry a tangent row into the pair loop: dmubar_j, u_j, ds_j (tangent_gauss).  ONE pass over the
// (emitter, sample, absorber) pairs, the exponent and its tangent side by side; every result is a store of 4 floats; no atomic add,
// no table: bitwise reproducible by construction.
//   ray_short_tangent_kernel  lane = ray.  One walk of the lane's list first leaves the three scalars per (list position, lane) in LDS,
//                             where the gradient kernel keeps its three running sums (grad_acc: 24 KB next to the 8 KB of lists); columns
//                             4..11 of a tangent row are read there, once, as two 16-byte loads per lane.  Then the radiance kernel's pair
//                             loop, chunked over emitters like ray_grad_chunk, rows one iteration ahead (grad_walk_begin / _next); columns
//                             0..3 of an emitter's row are read at its chunk, once, as the third 16-byte load.
//   ray_long_tangent_kernel   one wave per long ray, lane = emitter, the absorber wave-uniform and so its three scalars (scalar loads of
//                             its row); the four sums over the lanes by wave_sum in its fixed order, stored by one lane.
// A lane past the end of its list reads row 0 of the table and uses none of it (a select, not a product: the row may hold anything).
// Exp / Erf of the forward quantities are the selected pair's; e1 and e2 are exp_neg_sq<EXP>.  Only the four pairs of
// VRT_DISPATCH_GRAD_PAIR are instantiated; the entry point refuses the others.  Compiled with the default scheduler, like the gradient kernels.
#include "vrt_ray_grad.hpp"

namespace vrtk {

// The pair loop's body: EC emitters against one absorber q with the tangent scalars g (per lane in the short kernel, wave-uniform in
// the long): q's term of the exponents of T at the emitters' 5 EC sample points (grad_pass1's arithmetic) and of their tangents, and
// of F, the part of the tangent that no emitter and no sample point moves.
template <int EXP, int ERF, int EC>
__device__ __forceinline__ void tangent_pair(const ErfEval<ERF> &erf, const GradGauss &q, const TanGauss &g, const float (&e_mubar)[EC], const float (&e_sigma)[EC],
                                             const float (&e_dmubar)[EC], const float (&e_dsigma)[EC], float (&acc)[EC][5], float (&dacc)[EC][5], float &F)
{
    const float AC = q.A * ERF_SLOPE;
    const float dA = q.Am * g.u;
    F = __builtin_fmaf(AC * exp_neg_sq<EXP>(q.m), __builtin_fmaf(q.m, g.ds, -(g.dmubar * q.r)), F);
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const float base = __builtin_fmaf(e_mubar[e], q.r, -q.m);
        const float step = e_sigma[e] * q.r;
        const float dbase = (e_dmubar[e] - g.dmubar) * q.r;
        const float dstep = e_dsigma[e] * q.r;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float kf = (float)(k - 4);
            const float x = __builtin_fmaf(kf, step, base);
            const float D = q.E - erf(x);
            const float dx = __builtin_fmaf(-x, g.ds, __builtin_fmaf(kf, dstep, dbase));
            acc[e][k] = __builtin_fmaf(q.A, D, acc[e][k]);
            dacc[e][k] = __builtin_fmaf(dA, D, __builtin_fmaf(-(AC * exp_neg_sq<EXP>(x)), dx, dacc[e][k]));
        }
    }
}

// What an emitter adds to the ray's four sums once the exponents of its five samples and their tangents are known:
// t_k = sigma exp(acc_k - d2 / (2 sigma^2) - k^2 / 2) (grad_emitter's), V = sum_k t_k, and da m V + a (u V + m sum_k t_k (dacc_k + F)).
// A lane without this emitter adds exact zeros, whatever its rows held.
template <int EXP>
__device__ __forceinline__ void tangent_emit(bool on, float sigma, float d2, float inv2s2, float mag, float u, const float (&acc)[5], const float (&dacc)[5],
                                             float F, float4 alb, float4 dalb, float (&out)[4])
{
    float V = 0.f, TD = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float kf = (float)(k - 4);
        const float t = sigma * vexp<EXP>(acc[k] - d2 * inv2s2 - 0.5f * kf * kf);
        V += t;
        TD = __builtin_fmaf(t, dacc[k] + F, TD);
    }
    const float mV = on ? mag * V : 0.f;
    const float Z = on ? __builtin_fmaf(mag, TD, u * V) : 0.f;
    if (!on) { alb = make_float4(0.f, 0.f, 0.f, 0.f); dalb = alb; }
    out[0] += __builtin_fmaf(dalb.x, mV, alb.x * Z);
    out[1] += __builtin_fmaf(dalb.y, mV, alb.y * Z);
    out[2] += __builtin_fmaf(dalb.z, mV, alb.z * Z);
    out[3] += __builtin_fmaf(dalb.w, mV, alb.w * Z);
}
// columns 0..3 of row idx of the tangent table, or zeros without a table
__device__ __forceinline__ float4 tangent_albedo_load(const float *table, uint32_t idx)
{
    return table ? *(const float4 *)(table + (size_t)idx * GRAD_STRIDE) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// One chunk of EC emitters (list positions i0 .. i0+EC-1 of every lane) against the lane's whole list, one pass.  s_tan: the three
// scalars of every list position of the lane (grad_acc's layout: c = 0 dmubar, 1 u, 2 ds), zeros past the end of the lane's list.
template <int EXP, int ERF, int EC>
__device__ __forceinline__ void ray_tangent_chunk(const RayArgs *Pp, const SceneTables *Sp, const uint32_t *s_list /*[k*64 + lane]*/, float *s_tan, uint32_t nl,
                                                  uint32_t nmax, uint32_t lane, const LaneRay &ray, uint32_t i0, float (&out)[4])
{
    const SceneTables &S = *Sp;
    const ErfEval<ERF> erf;
    float e_mubar[EC], e_sigma[EC], e_dmubar[EC], e_dsigma[EC];
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const bool on = i0 + e < nl;
        const uint32_t idx = on ? s_list[(i0 + e) * 64 + lane] : 0u;
        grad_emitter_place(on, S.mu_sig[idx], ray, e_mubar[e], e_sigma[e]);
        e_dmubar[e] = on ? grad_acc(s_tan, 0, i0 + e, lane) : 0.f;
        e_dsigma[e] = on ? grad_acc(s_tan, 2, i0 + e, lane) * e_sigma[e] : 0.f;
    }
    float acc[EC][5], dacc[EC][5], F = 0.f;
#pragma unroll
    for (int e = 0; e < EC; ++e)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[e][k] = dacc[e][k] = 0.f;
    const LaneList L = { s_list, lane, nl, nmax };
    ListWalk lw = grad_walk_begin(S, L);
    for (uint32_t j = 0; j < nmax; ++j) {
        const GradGauss q = grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j);
        const TanGauss g = { grad_acc(s_tan, 0, j, lane), grad_acc(s_tan, 1, j, lane), grad_acc(s_tan, 2, j, lane) };
        tangent_pair<EXP>(erf, q, g, e_mubar, e_sigma, e_dmubar, e_dsigma, acc, dacc, F);
    }
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const bool on = i0 + e < nl;
        const uint32_t idx = on ? s_list[(i0 + e) * 64 + lane] : 0u;
        const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], on, ray);
        const float mag = on ? S.gD[idx].z : 0.f;
        const float u = on ? grad_acc(s_tan, 1, i0 + e, lane) : 0.f;
        tangent_emit<EXP>(on, e_sigma[e], q.d2, 0.5f * q.inv_s2, mag, u, acc[e], dacc[e], F, S.gC[idx], tangent_albedo_load(Pp->tangent, idx), out);
    }
}

template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_short_tangent_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    __shared__ float s_tan[3 * RAY_PL * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane); // the cull: exactly the radiance kernel's
    const uint32_t nl = R.nl, nmax = R.nmax;
    const LaneRay &ray = R.ray;
    const TanRay tr = tangent_ray(P.ray_tangent, R.rc);

    // ---- the tangent rows of the lane's list, each read once, to three scalars per position ----
    {
        const ErfEval<ERF> erf;
        const LaneList L = { s_list, lane, nl, nmax };
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
        }
    }

    float out[4] = { 0.f, 0.f, 0.f, 0.f };
    constexpr int EC = 4;
    for (uint32_t i0 = 0; i0 < nmax; i0 += EC) {
        const uint32_t rem = nmax - i0;
        if (rem >= (uint32_t)EC) ray_tangent_chunk<EXP, ERF, EC>(&P, &S, s_list, s_tan, nl, nmax, lane, ray, i0, out);
        else if (rem == 3) ray_tangent_chunk<EXP, ERF, 3>(&P, &S, s_list, s_tan, nl, nmax, lane, ray, i0, out);
        else if (rem == 2) ray_tangent_chunk<EXP, ERF, 2>(&P, &S, s_list, s_tan, nl, nmax, lane, ray, i0, out);
        else ray_tangent_chunk<EXP, ERF, 1>(&P, &S, s_list, s_tan, nl, nmax, lane, ray, i0, out);
    }
    if (R.writes) P.tangent_out[R.rc] = make_float4(out[0], out[1], out[2], out[3]); // a ray that keeps nothing: exact zeros
}

// One wave per long ray, lane = emitter (EC rounds of 64 at a time), the absorber wave-uniform.
template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_long_tangent_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    const ErfEval<ERF> erf;
    constexpr int EC = 2;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    LongRay L = ray_long_begin<SRC>(&P);
    while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) {
        const LaneRay ray = L.ray;
        const uint32_t n = L.n;
        const TanRay tr = tangent_ray(P.ray_tangent, L.r);
        float out[4] = { 0.f, 0.f, 0.f, 0.f }; // this lane's emitters; summed over the wave behind the rounds
        for (uint32_t e0 = 0; e0 < n; e0 += 64u * EC) {
            float e_mubar[EC], e_sigma[EC], e_dmubar[EC], e_dsigma[EC], e_u[EC];
            uint32_t e_idx[EC];
            bool e_on[EC];
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                const uint32_t p = e0 + (uint32_t)e * 64u + lane;
                e_on[e] = p < n;
                e_idx[e] = long_list_entry(s_list, L.slot, e_on[e] ? p : 0u);
                const float4 ms = S.mu_sig[e_idx[e]];
                grad_emitter_place(e_on[e], ms, ray, e_mubar[e], e_sigma[e]);
                const GradGauss q = grad_gauss<EXP, ERF>(erf, ms, S.gB[e_idx[e]], e_on[e], ray);
                float4 ms_t = zero4;
                float dm = 0.f;
                if (P.tangent) tangent_row_load(P.tangent, e_idx[e], ms_t, dm);
                const TanGauss g = tangent_gauss(q, ray, tr, e_on[e] ? S.gD[e_idx[e]].z : 0.f, ms_t, dm, e_on[e]);
                e_dmubar[e] = g.dmubar; e_dsigma[e] = g.ds * e_sigma[e]; e_u[e] = g.u;
            }
            float acc[EC][5], dacc[EC][5], F = 0.f;
#pragma unroll
            for (int e = 0; e < EC; ++e)
#pragma unroll
                for (int k = 0; k < 5; ++k) acc[e][k] = dacc[e][k] = 0.f;
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t idx = __builtin_amdgcn_readfirstlane(long_list_entry(s_list, L.slot, j));
                const GradGauss q = grad_gauss<EXP, ERF>(erf, uload(S.mu_sig, idx), uload(S.gB, idx), true, ray);
                float4 ms_t = zero4;
                float dm = 0.f;
                if (P.tangent) tangent_row_uload(P.tangent, idx, ms_t, dm);
                const TanGauss g = tangent_gauss(q, ray, tr, uload(S.gD, idx).z, ms_t, dm, true);
                tangent_pair<EXP>(erf, q, g, e_mubar, e_sigma, e_dmubar, e_dsigma, acc, dacc, F);
            }
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[e_idx[e]], S.gB[e_idx[e]], e_on[e], ray);
                const float mag = e_on[e] ? S.gD[e_idx[e]].z : 0.f;
                tangent_emit<EXP>(e_on[e], e_sigma[e], q.d2, 0.5f * q.inv_s2, mag, e_u[e], acc[e], dacc[e], F, S.gC[e_idx[e]],
                                  tangent_albedo_load(P.tangent, e_idx[e]), out);
            }
        }
        // ---- the lanes' shares in the wave's fixed order, one store ----
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = wave_sum(out[c]);
        if (lane == 0) P.tangent_out[L.r] = make_float4(out[0], out[1], out[2], out[3]);
    }
}

template <int EXP, int ERF>
static void launch_ray_tangent_bundle_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    if (src == RAY_LIST_PLAN) launch_ray_kernels(ray_short_tangent_kernel<EXP, ERF, RAY_LIST_PLAN>, ray_long_tangent_kernel<EXP, ERF, RAY_LIST_PLAN>, a, long_grid, st);
    else if (src == RAY_LIST_INDEX) launch_ray_kernels(ray_short_tangent_kernel<EXP, ERF, RAY_LIST_INDEX>, ray_long_tangent_kernel<EXP, ERF, RAY_LIST_INDEX>, a, long_grid, st);
    else launch_ray_kernels(ray_short_tangent_kernel<EXP, ERF, RAY_LIST_CHUNKS>, ray_long_tangent_kernel<EXP, ERF, RAY_LIST_CHUNKS>, a, long_grid, st);
}
void launch_ray_tangent_bundle(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !long_grid || !a.tangent_out || !ray_grad_pair_supported(exp_kind, erf_kind)) return;
    VRT_DISPATCH_GRAD_PAIR(launch_ray_tangent_bundle_t, a, long_grid, src, st);
}

} // namespace vrtk
