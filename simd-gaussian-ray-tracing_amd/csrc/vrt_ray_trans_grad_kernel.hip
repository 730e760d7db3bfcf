// vrt_ray_trans_grad_kernel.hip -- transmittance gradient bundles (vrt_hip_transmittance_bundle_grad*): d(loss) / d(mu, sigma,
// magnitude) of every Gaussian and d(loss) / d(sample), given d(loss) / d(T) at sample distances along caller-given rays -- or, in depth
// mode, d(loss) / d(Gaussians) and d(loss) / d(level), given d(loss) / d(depth) at the depths a depth bundle returned.  The rays, the
// cull, the lists, the queue of the long rays, the re-cull and the statistics are vrt_ray_cull.hpp's: the same rays keep the same
// Gaussians and go to the same kind of kernel as in every other bundle.  The kept list K of a ray is held fixed.
//
// The function ("Transmittance gradient bundles"; K = 1 / 0.79788456, C = 2 / sqrt(pi)):
//   A_j = K sigma_j mag_j exp(-d2_j / (2 sigma_j^2)),  x_kj = (s_k - mubar_j) r_j,  D_kj = Erf(-m_j) - Erf(x_kj),  m_j = mubar_j r_j
//   E_k = sum_j A_j D_kj,  T_k = Exp(E_k),  S_k = dE_k / ds_k = -sum_j A_j C r_j e2_kj,      e1_j = exp(-m_j^2), e2_kj = exp(-x_kj^2)
// and with a weight w_k per sample, W = sum_k w_k, P_j = sum_k w_k D_kj, Q_j = sum_k w_k e2_kj, R_j = sum_k w_k e2_kj x_kj:
//   d mag_j   = (A_j / mag_j) P_j
//   d mu_j    = -A_j P_j c_perp_j / sigma_j^2 + A_j C r_j (Q_j - e1_j W) n
//   d sigma_j = A_j P_j (1 / sigma_j + d2_j / sigma_j^3) + A_j C (e1_j m_j W + R_j) / sigma_j
// wrt == VRT_HIP_TGRAD_T:      g_k = dl / dT_k,      w_k = g_k T_k,    the per-sample output dl / ds_k   = w_k S_k
// wrt == VRT_HIP_TGRAD_DEPTH:  g_k = dl / ddepth_k,  w_k = -g_k / S_k, the per-sample output dl / dtau_k = g_k / (T_k S_k): the implicit
//   function theorem on T(depth, theta) = tau with dT / ds = T S -- the derivative of the IDEAL crossing, not of the upper end of the
//   bracket a depth bundle returns.  A sample whose s_k is not finite or <= 0, or whose S_k == 0 (the depth bundle's +inf, 0 and NaN
//   results) contributes exactly nothing, and its per-sample output is 0.
// In both modes a sample with g_k == 0 is skipped exactly (its s_k is never used: no 0 * NaN), per-sample output 0.
//   ray_short_trans_grad_kernel  lane = ray.  Per group of RAY_SG samples one walk of the lane's list (grad_walk_begin / grad_walk_next)
//                                forms E_k and S_k through grad_gauss (the compensated c and mubar, not trans_entry's |c|^2 - mubar^2),
//                                then w_k, then a second walk deals w_k out (grad_deal) to P, Q, R of every list position.  Three running
//                                sums per list position and lane in LDS (grad_acc: A P / mag, the coefficient of n without its W term,
//                                the sigma sum without its W term: 24 KB next to the 8 KB of lists).  Only W is carried beside them:
//                                e1_j comes back from grad_gauss.  After the last group every position goes to the table ONCE
//                                (grad_flush_short: grad_row_w, then the sink's deposit): 5 adds per (ray, kept Gaussian) whatever ns is,
//                                wave-summed where a position holds one row in all lanes.
//   ray_long_trans_grad_kernel   one wave per queued ray, lane l takes entries l, l + 64, ...  The list has no bound, so no per-entry
//                                sum waits in LDS: the samples are cut into chunks of NSC = 512.  E_k and S_k of a chunk's samples come
//                                from wave_sum (w_k is wave-uniform) and go to LDS with their s_k; then every lane runs over its entries
//                                with the chunk's samples in the inner loop (grad_deal), P, Q, R in registers, and adds its 5 values per
//                                entry and chunk (grad_row_w), the chunk's W terms included: 5 ceil(ns / NSC) adds per entry, every lane
//                                another row.
// The per-sample output is STORED (by the lane; by lane 0 of the long kernel), not added.
// RAYS (vrt_hip_transmittance_bundle_grad_rays*): d(loss) / d(origin, direction) of every ray as well, one stored row per ray, in either
// mode (the weights w_k are in the row segments already): grad_ray_add_w beside every grad_row_w, per lane in list order (short) or per
// lane over its entries and all chunks and then one wave_sum per component (long).  No atomic add; bitwise reproducible.  A template
// parameter: <.., false> is the kernel from before there were ray rows.
// Exp / Erf of the forward quantities are the selected pair's; e1 and e2 are exp_neg_sq<EXP>.  Only {vcl, libm} x {A&S, libm} are
// instantiated (ray_grad_pair_supported).  The sums in the caller's table depend on the arrival order of the atomic adds: not bitwise
// reproducible -- unless ORDERED (vrt_hip_set_grad_ordered): a template parameter of both kernels, instantiated in
// vrt_ray_trans_grad_ordered_kernel.hip.  Where a segment goes is GradSink's (vrt_ray_grad.hpp, with the record rules).
// Compiled with the default scheduler: nobody has measured -amdgpu-sched-strategy=max-ilp on these loops.
// What lives where: this file has what a sample is worth (trans_grad_weight; trans_grad_live and trans_grad_x are vrt_ray_grad.hpp's, shared with the tangent unit), the two kernels' loops over groups
// and chunks of samples, and the launch.  The helpers named above are vrt_ray_grad.hpp's, shared with vrt_ray_grad_kernel.hip.
#include "vrt_ray_grad.hpp"
#include "vrt_ray_trans.hpp" // RAY_SG

namespace vrtk {

constexpr int NSC = 512; // samples per chunk of the long kernel: their w_k and s_k in LDS (4 KB)
static_assert(NSC >= RAY_SG && NSC % RAY_SG == 0, "a chunk is whole groups");

// What a sample is worth once E_k and S_k = dE_k / ds_k are known: its weight w_k (0: it contributes nothing) and its per-sample output.
// g == 0: the sample is not live (trans_grad_live), whatever E and S_k came to.
template <int EXP>
__device__ __forceinline__ void trans_grad_weight(bool depth_mode, float g, float E, float Sk, float &w, float &gs)
{
    const bool live = g != 0.f;
    const float T = vexp<EXP>(E);
    if (depth_mode) {
        const bool ok = live && Sk != 0.f;
        w = ok ? -g / Sk : 0.f;
        gs = ok ? g / (T * Sk) : 0.f;
    } else {
        w = live ? g * T : 0.f;
        gs = live ? w * Sk : 0.f;
    }
}

// RAYS: the ray rows are asked for (P.grad_rays != nullptr); without, each kernel is the text it was before there were ray rows.
// ORDERED: one record per list position, the lane's own, opened and stored whole at the flush.  <.., false> is the kernel as it is without.
template <int EXP, int ERF, int SRC, bool RAYS, bool ORDERED = false>
__global__ __launch_bounds__(64) void ray_short_trans_grad_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    __shared__ float s_acc[3 * RAY_PL * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane); // the cull: exactly the radiance kernel's
    const uint32_t nl = R.nl, nmax = R.nmax;
    const LaneRay &ray = R.ray;
    const LaneList L = { s_list, lane, nl, nmax };
    const ErfEval<ERF> erf;
    const bool depth_mode = P.wrt == VRT_HIP_TGRAD_DEPTH;
    const uint64_t ns = P.ns;
    const float *sp = P.s + (P.s_per_ray ? R.rc * ns : 0ull);
    const float *gp = P.grad_T + R.rc * ns;
    float *gsp = P.grad_s ? P.grad_s + R.rc * ns : nullptr;

    for (uint32_t p = 0; p < nmax; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c) grad_acc(s_acc, c, p, lane) = 0.f; // here: A P / mag, A C r Q, A C R / sigma

    float W = 0.f;
    for (uint64_t k0 = 0; k0 < ns; k0 += RAY_SG) {
        float sv[RAY_SG], gv[RAY_SG], w[RAY_SG];
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g) {
            const bool in = R.writes && k0 + g < ns;
            const float g_in = in ? gp[k0 + g] : 0.f, s = in ? sp[k0 + g] : 0.f;
            gv[g] = trans_grad_live(depth_mode, s, g_in) ? g_in : 0.f;
            sv[g] = gv[g] != 0.f ? s : 0.f;
        }
        // ---- walk 1: E_k and S_k ----
        float accE[RAY_SG], accS[RAY_SG];
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g) accE[g] = accS[g] = 0.f;
        ListWalk lw = grad_walk_begin(S, L);
        for (uint32_t j = 0; j < nmax; ++j) {
            const bool vj = L.has(j);
            const GradGauss q = grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j);
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) {
                const float x = trans_grad_x(sv[g], q);
                const float e = __builtin_fmaf(q.A, q.E - erf(x), accE[g]);
                const float t = __builtin_fmaf(-q.Ar, exp_neg_sq<EXP>(x), accS[g]);
                accE[g] = vj ? e : accE[g];
                accS[g] = vj ? t : accS[g];
            }
        }
        // ---- the samples: w_k, and what leaves per sample ----
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g) {
            float gs;
            trans_grad_weight<EXP>(depth_mode, gv[g], accE[g], accS[g], w[g], gs);
            W += w[g];
            if (gsp && R.writes && k0 + g < ns) gsp[k0 + g] = gs;
        }
        if (!RAYS && !P.grad) continue;
        // ---- walk 2: the same entries again; w_k to P, Q, R of every position ----
        lw = grad_walk_begin(S, L);
        for (uint32_t j = 0; j < nmax; ++j) {
            const GradGauss q = grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j);
            float Pj = 0.f, Qj = 0.f, Rj = 0.f;
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) grad_deal<EXP>(erf, w[g], trans_grad_x(sv[g], q), q.E, Pj, Qj, Rj);
            if (L.has(j)) {
                grad_acc(s_acc, 0, j, lane) += q.Am * Pj;
                grad_acc(s_acc, 1, j, lane) += q.Ar * Qj;
                grad_acc(s_acc, 2, j, lane) += q.Ar * Rj * SQRT_2;
            }
        }
    }
    GradSink<ORDERED> sink(&P, true);
    sink.short_ray(R);
    if (RAYS || sink.table()) grad_flush_short<EXP, ERF, RAYS>(sink, P.grad_rays, R.rc, R.writes, S, erf, L, s_acc, ray, W);
}

// One wave per long ray, lane l takes entries l, l + 64, ...; the samples in chunks of NSC.
// ORDERED: one record per entry, record p owned by the lane that takes entry p: opened with the first chunk of samples, the later chunks'
// segments added onto the lane's own stores.
template <int EXP, int ERF, int SRC, bool RAYS, bool ORDERED = false>
__global__ __launch_bounds__(64) void ray_long_trans_grad_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    __shared__ float s_w[NSC], s_s[NSC]; // the chunk's g_k, then its weights w_k, and the distances they are formed at
    const uint32_t lane = threadIdx.x & 63u;
    const ErfEval<ERF> erf;
    const bool depth_mode = P.wrt == VRT_HIP_TGRAD_DEPTH;
    const uint64_t ns = P.ns;

    LongRay L = ray_long_begin<SRC>(&P);
    while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) {
        const LaneRay ray = L.ray;
        const uint32_t n = L.n;
        const float *sp = P.s + (P.s_per_ray ? L.r * ns : 0ull);
        const float *gp = P.grad_T + L.r * ns;
        float *gsp = P.grad_s ? P.grad_s + L.r * ns : nullptr;
        GradSink<ORDERED> sink(&P, true); // per ray: built outside, the range's base is carried round this loop (profiles/grad_sink_refactor.md)
        if (!sink.long_ray(L.r, n, 1u, lane)) continue;
        [[maybe_unused]] float go[3] = { 0.f, 0.f, 0.f }, gn[3] = { 0.f, 0.f, 0.f }; // this lane's shares of the ray's row, over its entries and all chunks
        for (uint64_t c0 = 0; c0 < ns; c0 += NSC) {
            const uint32_t nc = (uint32_t)(ns - c0 < (uint64_t)NSC ? ns - c0 : (uint64_t)NSC);
            // ---- the chunk's samples to LDS, lane = sample (whole groups: what lies past the end is not live) ----
            for (uint32_t k = lane; k < ((nc + RAY_SG - 1u) & ~(uint32_t)(RAY_SG - 1)); k += 64u) {
                const bool in = k < nc;
                const float g_in = in ? gp[c0 + k] : 0.f, s = in ? sp[c0 + k] : 0.f;
                const float g = trans_grad_live(depth_mode, s, g_in) ? g_in : 0.f;
                s_w[k] = g; s_s[k] = g != 0.f ? s : 0.f;
            }
            __syncthreads();
            // ---- E_k, S_k and w_k of the chunk's samples, RAY_SG per walk of the list; w_k takes the place of g_k ----
            float Wc = 0.f;
            for (uint32_t k0 = 0; k0 < nc; k0 += RAY_SG) {
                float sv[RAY_SG], gv[RAY_SG], accE[RAY_SG], accS[RAY_SG];
#pragma unroll
                for (int g = 0; g < RAY_SG; ++g) {
                    gv[g] = s_w[k0 + g]; sv[g] = s_s[k0 + g]; // k0 + g < NSC: a chunk is whole groups
                    accE[g] = accS[g] = 0.f;
                }
                for (uint32_t p = lane; p < n; p += 64u) {
                    const uint32_t idx = long_list_entry(s_list, L.slot, p);
                    const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], true, ray);
#pragma unroll
                    for (int g = 0; g < RAY_SG; ++g) {
                        const float x = trans_grad_x(sv[g], q);
                        accE[g] = __builtin_fmaf(q.A, q.E - erf(x), accE[g]);
                        accS[g] = __builtin_fmaf(-q.Ar, exp_neg_sq<EXP>(x), accS[g]);
                    }
                }
#pragma unroll
                for (int g = 0; g < RAY_SG; ++g) { // the whole wave is here again
                    const float E = wave_sum(accE[g]), Sk = wave_sum(accS[g]);
                    float w, gs;
                    trans_grad_weight<EXP>(depth_mode, gv[g], E, Sk, w, gs);
                    Wc += w;
                    if (lane == 0) {
                        s_w[k0 + g] = w;
                        if (gsp && k0 + g < nc) gsp[c0 + k0 + g] = gs;
                    }
                }
            }
            __syncthreads(); // the chunk's weights are in LDS
            // ---- every lane its entries, the chunk's samples in the inner loop ----
            if (RAYS || sink.table()) {
                for (uint32_t p = lane; p < n; p += 64u) {
                    const uint32_t idx = long_list_entry(s_list, L.slot, p);
                    const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], true, ray);
                    float Pj = 0.f, Qj = 0.f, Rj = 0.f;
#pragma unroll 4
                    for (uint32_t k = 0; k < nc; ++k) grad_deal<EXP>(erf, s_w[k], trans_grad_x(s_s[k], q), q.E, Pj, Qj, Rj);
                    const float mag = S.gD[idx].z;
                    if constexpr (RAYS) grad_ray_add_w<EXP>(q, ray, mag, q.Am * Pj, q.Ar * Qj, Wc, go, gn);
                    if (sink.table()) {
                        float d[5];
                        grad_row_w<EXP>(q, ray, mag, q.Am * Pj, q.Ar * Qj, q.Ar * Rj * SQRT_2, Wc, d);
                        sink.template put<5>(p, idx, 4u, d, GRAD_OPEN, c0 == 0);
                    }
                }
            }
            __syncthreads(); // the chunk's weights are read before the next chunk's are written
        }
        // ---- the ray's row: the lanes' shares in the wave's fixed order, one store ----
        if constexpr (RAYS) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { go[c] = wave_sum(go[c]); gn[c] = wave_sum(gn[c]); }
            if (lane == 0) grad_ray_store(P.grad_rays, L.r, go, gn);
        }
    }
}

#ifndef VRT_GRAD_ORDERED_UNIT
template <int EXP, int ERF>
static void launch_ray_trans_grad_bundle_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    grad_dispatch_source_rays(src, a.grad_rays != nullptr, [&](auto I, auto R) {
        launch_ray_kernels(ray_short_trans_grad_kernel<EXP, ERF, I.value, R.value, false>, ray_long_trans_grad_kernel<EXP, ERF, I.value, R.value, false>, a, long_grid, st);
    });
}
void launch_ray_trans_grad_bundle(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !a.ns || !long_grid || !ray_grad_pair_supported(exp_kind, erf_kind)) return;
    VRT_DISPATCH_GRAD_PAIR(launch_ray_trans_grad_bundle_t, a, long_grid, src, st);
}
#else // vrt_ray_trans_grad_ordered_kernel.hip: the ORDERED instantiations alone, so that the build stays parallel
template <int EXP, int ERF>
static void launch_ray_trans_grad_bundle_ordered_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    grad_dispatch_source_rays(src, a.grad_rays != nullptr, [&](auto I, auto R) {
        launch_ray_kernels(ray_short_trans_grad_kernel<EXP, ERF, I.value, R.value, true>, ray_long_trans_grad_kernel<EXP, ERF, I.value, R.value, true>, a, long_grid, st);
    });
}
void launch_ray_trans_grad_bundle_ordered(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !a.ns || !long_grid || !a.grad || !ray_grad_pair_supported(exp_kind, erf_kind)) return;
    VRT_DISPATCH_GRAD_PAIR(launch_ray_trans_grad_bundle_ordered_t, a, long_grid, src, st);
}
#endif

} // namespace vrtk
