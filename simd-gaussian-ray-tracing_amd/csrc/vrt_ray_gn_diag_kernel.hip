// vrt_ray_gn_diag_kernel.hip -- Gauss-Newton diagonal bundles (vrt_hip_radiance_rays_gn_diag*): for every Gaussian parameter theta
//   D[theta] = sum over rays r and channels c of wt[r, c] (d L_c(r) / d theta)^2,
// the diagonal of J^T W J of the radiance of caller-given rays.  The rays, the cull, the lists, the queue of the long rays, the re-cull
// and the statistics are vrt_ray_cull.hpp's; L, the kept list held fixed and the analytic derivatives are the gradient bundle's
// (vrt_ray_grad_kernel.hip states them, DESIGN.md section 4 "Gauss-Newton diagonal bundles" the rest).
//
// The row of channel c is the gradient bundle's row for g = e_c: there the channel enters through G_i = a_ic alone, a factor on the
// weights w_ik = a_ic m_i t_ik (t_ik: the ik term of L without albedo and magnitude).  So both pair loops run ONCE for the four rows, on
// w = m t: per (emitter, absorber) pair the scalar sums p, q, r of grad_deal, spread over the channels by the emitter's albedo
// (gn_pass2, grad_spread); z_i, y_i, V_i and W spread the same way.  What separates this from the gradient kernels: a row is squared PER
// RAY, so it must be complete -- all emitter chunks, and the terms in W_c -- before it leaves, and nothing partial can go to the table.
//   ray_short_gn_diag_kernel  lane = ray.  Twelve running sums per list position and lane in LDS (gn_acc: 96 KB next to the 8 KB of
//                             lists, one one-wave workgroup per CU) take the chunks' shares; the flush forms the four rows per position
//                             (grad_row_w as it stands), squares, weights and sums them (gn_rows_squared) and hands ONE segment to the
//                             sink.  The albedo columns wt_c (m V)^2 are complete at the emitter's chunk and leave there.
//   ray_long_gn_diag_kernel   one wave per ray, lane = emitter, the absorber wave-uniform.  The twelve sums of list position p belong to
//                             lane p mod 64 from the first round to the last walk: in LDS for p < RAY_LCAP (48 KB), beyond that in the
//                             workgroup's slot of the workspace in device memory (RayArgs::gn_work) -- plain loads and stores of the
//                             owning lane, no atomics.  Per (round, absorber) the twelve sums over the wave go to the absorber's owner;
//                             an emitter's own terms are its owner's anyway.  The last walk (lane = position) finishes, squares and
//                             hands over.
// Deposits go through GradSink: float atomic adds of the segments (non-negative under non-negative weights), or -- ORDERED
// (vrt_hip_set_grad_ordered; vrt_ray_gn_diag_ordered_kernel.hip) -- ONE record per (ray, kept Gaussian) in either kernel: the ray's own
// share of D.  Only the pairs of ray_grad_pair_supported are instantiated.  Compiled with the default scheduler, as the gradient kernels.
#include "vrt_ray_grad.hpp"

namespace vrtk {

// s_acc of the short kernel: [(c * RAY_PL + pos) * 64 + lane], c < GN_SUMS
__device__ __forceinline__ float &gn_acc(float *s_acc, int c, uint32_t pos, uint32_t lane) { return s_acc[((uint32_t)c * RAY_PL + pos) * 64u + lane]; }

__device__ __forceinline__ void gn_load_weights(const RayArgs *Pp, uint64_t r, float (&wt)[4])
{
    if (Pp->gn_weights) { // wave-uniform
        const float4 v = Pp->gn_weights[r];
        wt[0] = v.x; wt[1] = v.y; wt[2] = v.z; wt[3] = v.w;
    } else wt[0] = wt[1] = wt[2] = wt[3] = 1.f;
}

// One emitter behind pass 1: w = m t, V, its albedo (exact zeros in a lane without it), the shares of the four W, and the albedo columns
template <int EXP, int ERF>
__device__ __forceinline__ float gn_emitter(const SceneTables &S, const ErfEval<ERF> &erf, bool on, uint32_t idx, float e_sigma, const LaneRay &ray, const float (&acc)[5],
                                            const float (&wt)[4], float (&w)[5], float (&alb)[4], float (&W)[4], float (&da)[4])
{
    const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], on, ray);
    const float4 a = S.gC[idx];
    const float mag = on ? S.gD[idx].z : 0.f;
    alb[0] = on ? a.x : 0.f; alb[1] = on ? a.y : 0.f; alb[2] = on ? a.z : 0.f; alb[3] = on ? a.w : 0.f;
    const float V = grad_emitter<EXP>(on, e_sigma, q.d2, 0.5f * q.inv_s2, mag, acc, w);
    const float mV = mag * V;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        W[c] = __builtin_fmaf(alb[c] * V, mag, W[c]);
        da[c] = wt[c] * mV * mV;
    }
    return V;
}

// One chunk of EC emitters against the lane's whole list, both passes, as ray_grad_chunk -- for the four channels at once
template <int EXP, int ERF, int EC, bool ORDERED>
__device__ __forceinline__ void ray_gn_chunk(const GradSink<ORDERED> &sink, const SceneTables *Sp, const uint32_t *s_list /*[k*64 + lane]*/, float *s_acc, uint32_t nl,
                                             uint32_t nmax, uint32_t lane, const LaneRay &ray, uint32_t i0, const float (&wt)[4], float (&W)[4])
{
    const SceneTables &S = *Sp;
    const ErfEval<ERF> erf;
    float e_mubar[EC], e_sigma[EC];
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const bool on = i0 + e < nl;
        const uint32_t idx = on ? s_list[(i0 + e) * 64 + lane] : 0u;
        grad_emitter_place(on, S.mu_sig[idx], ray, e_mubar[e], e_sigma[e]);
    }

    // ---- pass 1: the exponents of T at the chunk's 5 EC sample points ----
    float acc[EC][5];
#pragma unroll
    for (int e = 0; e < EC; ++e)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[e][k] = 0.f;
    const LaneList L = { s_list, lane, nl, nmax };
    ListWalk lw = grad_walk_begin(S, L);
    for (uint32_t j = 0; j < nmax; ++j) grad_pass1(erf, grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j), e_mubar, e_sigma, acc);

    // ---- the emitters: w_ik = m t_ik, V_i, the albedo; the albedo columns are complete and leave here ----
    float w[EC][5], alb[EC][4], V[EC];
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const bool on = i0 + e < nl;
        const uint32_t idx = on ? s_list[(i0 + e) * 64 + lane] : 0u;
        float da[4];
        V[e] = gn_emitter<EXP, ERF>(S, erf, on, idx, e_sigma[e], ray, acc[e], wt, w[e], alb[e], W, da);
        sink.template deposit<4>((uint64_t)i0 + e, idx, on, da, 0u, lane, GRAD_STORE);
    }

    // ---- pass 2: the same pairs again, the scalar sums spread over the channels ----
    float z[EC], y[EC];
#pragma unroll
    for (int e = 0; e < EC; ++e) z[e] = y[e] = 0.f;
    lw = grad_walk_begin(S, L);
    for (uint32_t j = 0; j < nmax; ++j) {
        const GradGauss q = grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j);
        float Pc[4] = { 0.f, 0.f, 0.f, 0.f }, Qc[4] = { 0.f, 0.f, 0.f, 0.f }, Rc[4] = { 0.f, 0.f, 0.f, 0.f };
        gn_pass2<EXP>(erf, q, e_mubar, e_sigma, w, alb, z, y, Pc, Qc, Rc);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            gn_acc(s_acc, 3 * c, j, lane) += q.Am * Pc[c];
            gn_acc(s_acc, 3 * c + 1, j, lane) += q.Ar * Qc[c];
            gn_acc(s_acc, 3 * c + 2, j, lane) += q.Ar * Rc[c] * SQRT_2;
        }
    }
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        if (i0 + e < nl) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                gn_acc(s_acc, 3 * c, i0 + e, lane) += alb[e][c] * V[e];
                gn_acc(s_acc, 3 * c + 1, i0 + e, lane) -= alb[e][c] * z[e];
                gn_acc(s_acc, 3 * c + 2, i0 + e, lane) -= alb[e][c] * y[e];
            }
        }
    }
}

// ORDERED: one record per list position, the lane's own -- the albedo columns at the emitter's chunk, columns 4..8 and the name at the flush.
template <int EXP, int ERF, int SRC, bool ORDERED = false>
__global__ __launch_bounds__(64) void ray_short_gn_diag_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]
    __shared__ float s_acc[GN_SUMS * RAY_PL * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane); // the cull: exactly the radiance kernel's
    const uint32_t nl = R.nl, nmax = R.nmax;
    const LaneRay &ray = R.ray;
    float wt[4];
    gn_load_weights(&P, R.rc, wt);
    GradSink<ORDERED> sink(&P, false);
    sink.short_ray(R);

    for (uint32_t p = 0; p < nmax; ++p)
#pragma unroll
        for (int c = 0; c < GN_SUMS; ++c) gn_acc(s_acc, c, p, lane) = 0.f;

    float W[4] = { 0.f, 0.f, 0.f, 0.f };
    constexpr int EC = 4;
    for (uint32_t i0 = 0; i0 < nmax; i0 += EC) {
        const uint32_t rem = nmax - i0;
        if (rem >= (uint32_t)EC) ray_gn_chunk<EXP, ERF, EC>(sink, &S, s_list, s_acc, nl, nmax, lane, ray, i0, wt, W);
        else if (rem == 3) ray_gn_chunk<EXP, ERF, 3>(sink, &S, s_list, s_acc, nl, nmax, lane, ray, i0, wt, W);
        else if (rem == 2) ray_gn_chunk<EXP, ERF, 2>(sink, &S, s_list, s_acc, nl, nmax, lane, ray, i0, wt, W);
        else ray_gn_chunk<EXP, ERF, 1>(sink, &S, s_list, s_acc, nl, nmax, lane, ray, i0, wt, W);
    }

    // ---- every position is complete: four rows each, squared, one segment to the sink (position p: record p, opened here) ----
    const ErfEval<ERF> erf;
    const LaneList L = { s_list, lane, nl, nmax };
    for (uint32_t p = 0; p < nmax; ++p) {
        const bool on = L.has(p);
        const uint32_t idx = L.at(p);
        const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], on, ray);
        const float mag = on ? S.gD[idx].z : 0.f;
        float sums[GN_SUMS], d[5];
#pragma unroll
        for (int c = 0; c < GN_SUMS; ++c) sums[c] = gn_acc(s_acc, c, p, lane);
        gn_rows_squared<EXP>(q, ray, mag, sums, W, wt, d);
        sink.template deposit<5>(p, idx, on, d, 4u, lane, GRAD_OPEN);
    }
}

// the twelve sums of position p of a long ray: LDS below RAY_LCAP ([c * RAY_LCAP + p]), the workgroup's workspace slot from there on
__device__ __forceinline__ float gn_long_get(const float *s_sum, const float *work, uint32_t p, int c)
{
    return p < (uint32_t)RAY_LCAP ? s_sum[(uint32_t)c * RAY_LCAP + p] : work[(size_t)(p - (uint32_t)RAY_LCAP) * GN_SUMS + c];
}
__device__ __forceinline__ void gn_long_set(float *s_sum, float *work, uint32_t p, int c, float v)
{
    if (p < (uint32_t)RAY_LCAP) s_sum[(uint32_t)c * RAY_LCAP + p] = v;
    else work[(size_t)(p - (uint32_t)RAY_LCAP) * GN_SUMS + c] = v;
}

// One wave per long ray.  Position p's sums, its record (ORDERED: record p, one per kept Gaussian) and its deposits are lane p mod 64's.
template <int EXP, int ERF, int SRC, bool ORDERED = false>
__global__ __launch_bounds__(64) void ray_long_gn_diag_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    __shared__ float s_sum[GN_SUMS * RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    const ErfEval<ERF> erf;
    constexpr int EC = 2;
    GradSink<ORDERED> sink(&P, false);
    float *work = P.gn_work + (size_t)blockIdx.x * P.gn_work_slot; // touched only for p >= RAY_LCAP, which takes S.n > RAY_LCAP

    LongRay L = ray_long_begin<SRC>(&P);
    while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) {
        const LaneRay ray = L.ray;
        const uint32_t n = L.n;
        if (!sink.long_ray(L.r, n, 1u, lane)) continue;
        float wt[4];
        gn_load_weights(&P, L.r, wt);
        for (uint32_t p = lane; p < n; p += 64u)
#pragma unroll
            for (int c = 0; c < GN_SUMS; ++c) gn_long_set(s_sum, work, p, c, 0.f);
        float W[4] = { 0.f, 0.f, 0.f, 0.f }; // this lane's emitters; summed over the wave behind the rounds
        for (uint32_t e0 = 0; e0 < n; e0 += 64u * EC) {
            float e_mubar[EC], e_sigma[EC];
            uint32_t e_idx[EC];
            bool e_on[EC];
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                const uint32_t p = e0 + (uint32_t)e * 64u + lane;
                e_on[e] = p < n;
                e_idx[e] = long_list_entry(s_list, L.slot, e_on[e] ? p : 0u);
                grad_emitter_place(e_on[e], S.mu_sig[e_idx[e]], ray, e_mubar[e], e_sigma[e]);
            }
            // ---- pass 1 ----
            float acc[EC][5];
#pragma unroll
            for (int e = 0; e < EC; ++e)
#pragma unroll
                for (int k = 0; k < 5; ++k) acc[e][k] = 0.f;
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t idx = __builtin_amdgcn_readfirstlane(long_list_entry(s_list, L.slot, j));
                grad_pass1(erf, grad_gauss<EXP, ERF>(erf, uload(S.mu_sig, idx), uload(S.gB, idx), true, ray), e_mubar, e_sigma, acc);
            }
            // ---- the emitters; the albedo columns open the position's record ----
            float w[EC][5], alb[EC][4], V[EC];
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                float da[4];
                V[e] = gn_emitter<EXP, ERF>(S, erf, e_on[e], e_idx[e], e_sigma[e], ray, acc[e], wt, w[e], alb[e], W, da);
                if (e_on[e]) sink.template put<4>((uint64_t)e0 + (uint32_t)e * 64u + lane, e_idx[e], 0u, da, GRAD_OPEN);
            }
            // ---- pass 2: per absorber the twelve sums over the wave, to the absorber's owner ----
            float z[EC], y[EC];
#pragma unroll
            for (int e = 0; e < EC; ++e) z[e] = y[e] = 0.f;
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t idx = __builtin_amdgcn_readfirstlane(long_list_entry(s_list, L.slot, j));
                const GradGauss q = grad_gauss<EXP, ERF>(erf, uload(S.mu_sig, idx), uload(S.gB, idx), true, ray);
                float Pc[4] = { 0.f, 0.f, 0.f, 0.f }, Qc[4] = { 0.f, 0.f, 0.f, 0.f }, Rc[4] = { 0.f, 0.f, 0.f, 0.f };
                gn_pass2<EXP>(erf, q, e_mubar, e_sigma, w, alb, z, y, Pc, Qc, Rc);
#pragma unroll
                for (int c = 0; c < 4; ++c) { Pc[c] = wave_sum(Pc[c]); Qc[c] = wave_sum(Qc[c]); Rc[c] = wave_sum(Rc[c]); }
                if (lane == (j & 63u)) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        gn_long_set(s_sum, work, j, 3 * c, gn_long_get(s_sum, work, j, 3 * c) + q.Am * Pc[c]);
                        gn_long_set(s_sum, work, j, 3 * c + 1, gn_long_get(s_sum, work, j, 3 * c + 1) + q.Ar * Qc[c]);
                        gn_long_set(s_sum, work, j, 3 * c + 2, gn_long_get(s_sum, work, j, 3 * c + 2) + q.Ar * Rc[c] * SQRT_2);
                    }
                }
            }
            // ---- the emitters' own terms: every lane its own position ----
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                if (e_on[e]) {
                    const uint32_t p = e0 + (uint32_t)e * 64u + lane;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        gn_long_set(s_sum, work, p, 3 * c, gn_long_get(s_sum, work, p, 3 * c) + alb[e][c] * V[e]);
                        gn_long_set(s_sum, work, p, 3 * c + 1, gn_long_get(s_sum, work, p, 3 * c + 1) - alb[e][c] * z[e]);
                        gn_long_set(s_sum, work, p, 3 * c + 2, gn_long_get(s_sum, work, p, 3 * c + 2) - alb[e][c] * y[e]);
                    }
                }
            }
        }
        // ---- W is known: lane = list position finishes its rows, squares them and hands the segment over ----
#pragma unroll
        for (int c = 0; c < 4; ++c) W[c] = wave_sum(W[c]);
        for (uint32_t p0 = 0; p0 < n; p0 += 64u) {
            const uint32_t p = p0 + lane;
            if (p < n) {
                const uint32_t idx = long_list_entry(s_list, L.slot, p);
                const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], true, ray);
                float sums[GN_SUMS], d[5];
#pragma unroll
                for (int c = 0; c < GN_SUMS; ++c) sums[c] = gn_long_get(s_sum, work, p, c);
                gn_rows_squared<EXP>(q, ray, S.gD[idx].z, sums, W, wt, d);
                sink.template put<5>(p, idx, 4u, d, GRAD_STORE);
            }
        }
    }
}

#ifndef VRT_GN_DIAG_ORDERED_UNIT
template <int EXP, int ERF>
static void launch_ray_gn_diag_bundle_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    grad_dispatch_source(src, [&](auto I) {
        launch_ray_kernels(ray_short_gn_diag_kernel<EXP, ERF, I.value, false>, ray_long_gn_diag_kernel<EXP, ERF, I.value, false>, a, long_grid, st);
    });
}
void launch_ray_gn_diag_bundle(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    long_grid = std::min(long_grid, a.gn_grid);
    if (!a.nrays || !long_grid || !a.grad || !ray_grad_pair_supported(exp_kind, erf_kind)) return;
    VRT_DISPATCH_GRAD_PAIR(launch_ray_gn_diag_bundle_t, a, long_grid, src, st);
}

#else // vrt_ray_gn_diag_ordered_kernel.hip: the ORDERED instantiations alone, so that the build stays parallel
template <int EXP, int ERF>
static void launch_ray_gn_diag_bundle_ordered_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    grad_dispatch_source(src, [&](auto I) {
        launch_ray_kernels(ray_short_gn_diag_kernel<EXP, ERF, I.value, true>, ray_long_gn_diag_kernel<EXP, ERF, I.value, true>, a, long_grid, st);
    });
}
void launch_ray_gn_diag_bundle_ordered(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    long_grid = std::min(long_grid, a.gn_grid);
    if (!a.nrays || !long_grid || !a.grad || !ray_grad_pair_supported(exp_kind, erf_kind)) return;
    VRT_DISPATCH_GRAD_PAIR(launch_ray_gn_diag_bundle_ordered_t, a, long_grid, src, st);
}
#endif

} // namespace vrtk
