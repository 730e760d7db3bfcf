// vrt_ray_grad_kernel.hip -- gradient bundles (vrt_hip_radiance_rays_grad*): d(loss) / d(albedo, mu, sigma, magnitude) of every Gaussian,
// given d(loss) / d(radiance) of caller-given rays.  The rays, the cull, the lists, the queue of the long rays, the re-cull and the
// statistics are vrt_ray_cull.hpp's, the text the radiance kernels of vrt_ray_kernel.hip run: the same rays keep the same Gaussians and
// go to the same kind of kernel.  The kept list K of a ray is held fixed (the cull is piecewise constant in the parameters).
//
// The function ("Gradient bundles"; K = 1 / 0.79788456 as everywhere in this library, C = 2 / sqrt(pi)):
//   A_j = K sigma_j m_j exp(-d2_j / (2 sigma_j^2)),  x_ikj = (mubar_i + k sigma_i - mubar_j) r_j,  D_ikj = Erf(-mubar_j r_j) - Erf(x_ikj),
//   T_ik = Exp(sum_j A_j D_ikj),  L = sum_i a_i sum_k sigma_i m_i exp(-d2_i / (2 sigma_i^2) - k^2 / 2) T_ik,           k = -4..0
// and with g = dl/dL, G_i = g . a_i, w_ik = G_i (the ik term of L), W = sum_ik w_ik and per absorber j the three sums
//   P_j = sum_ik w_ik D_ikj,   Q_j = sum_ik w_ik e2_ikj,   R_j = sum_ik w_ik e2_ikj x_ikj,      e2 = exp(-x^2), e1_j = exp(-(mubar_j r_j)^2)
// the contributions (to the emitter, to the emitter through its sample points, to every absorber) collapse to
//   d m_j     = M_j            = (A_j / m_j) P_j + G_j V_j                         V_j = sum_k (the jk term of L) / m_j, formed without m_j
//   d mu_j    = -m_j M_j c_perp_j / sigma_j^2 + [A_j C r_j (Q_j - e1_j W) + Z_j] n        Z_j = sum_k w_jk S_jk = -sum_i C A_i r_i sum_k w_jk e2_jki
//   d sigma_j = m_j M_j (1 / sigma_j + d2_j / sigma_j^3) + A_j C (e1_j mubar_j r_j W + R_j) / sigma_j + Y_j          Y_j = sum_k k w_jk S_jk
//   d a_j     = g m_j V_j
// Two passes over the pair loop per emitter chunk: the first is the radiance kernels' (the exponents of T, then w_ik); the second
// evaluates D and e2 again and deals w_ik out to the absorbers (P, Q, R) and, through the same products, back to the emitter (Z, Y).
// Nothing of size 5 n is stored: a chunk's w_ik live in registers between its two passes.
//   ray_short_grad_kernel  lane = ray.  Three running sums per list position and lane in LDS (grad_acc: M, the n coefficient, the sigma
//                          sum: 24 KB next to the 8 KB of lists) take the chunks' shares (ray_grad_chunk: two walks of the lane's list
//                          through grad_walk_begin / grad_walk_next, their bodies grad_pass1 and grad_pass2); when all chunks are
//                          through, W is known and every position is dealt to the caller's table once (grad_flush_short: grad_row_w,
//                          then the sink's deposit): 9 atomic adds per (ray, kept Gaussian) -- 4 (albedo) behind the emitter's chunk, 5 at the
//                          end.  Where a position holds the same scene index in every lane that has one (a coherent bundle), the values
//                          are summed over the wave (wave_sum) and ONE row segment is added.
//   ray_long_grad_kernel   one wave per ray, lane = emitter, the absorber wave-uniform: the same grad_pass1 and grad_pass2; P, Q, R are
//                          summed over the wave per (round of 128 emitters, absorber) and lanes 0..4 add one row segment (grad_row); the
//                          emitter's own terms (grad_row again) are per-lane adds (every lane another row); the terms in W follow in a
//                          last walk of the list.
// Exp / Erf of the forward quantities are the selected pair's; e1 and e2 are exp_neg_sq<EXP>.  Only {vcl, libm} x {A&S, libm} are
// instantiated: the piecewise approximations have jumps, and the entry point refuses them.
// The sums in the caller's table depend on the arrival order of the atomic adds: not bitwise reproducible -- unless ORDERED
// (vrt_hip_set_grad_ordered): a template parameter of both kernels, instantiated in vrt_ray_grad_ordered_kernel.hip.  Where a segment
// goes is GradSink's (vrt_ray_grad.hpp, with the record rules); the kernels say which lane owns which record and when a write is the first.
// RAYS (vrt_hip_radiance_rays_grad_rays*): d(loss) / d(origin, direction) of every ray as well, one stored row per ray (grad_ray_add of
// vrt_ray_grad.hpp beside every grad_row; DESIGN.md section 4, "Ray gradients"): summed per lane in list order (short) or per lane and then
// over the wave in its fixed order (long), no atomic add, bitwise reproducible.  With RAYS the table may be missing (P.grad == nullptr): no
// table add is issued.  RAYS is a template parameter: <.., false> is the kernel from before there were ray rows, register for register.
// Compiled with the default scheduler: nobody has measured -amdgpu-sched-strategy=max-ilp on these loops.
// What lives where: this file has the chunk of the short kernel, the two kernels' own loops -- how
// the absorber is loaded (per lane; readfirstlane + uload) and where a sum goes (LDS; the sink) -- and the launch.  Every formula named
// above is vrt_ray_grad.hpp's, shared with vrt_ray_trans_grad_kernel.hip.
#include "vrt_ray_grad.hpp"

namespace vrtk {

// One chunk of EC emitters (list positions i0 .. i0+EC-1 of every lane) against the lane's whole list, both passes.  The albedo
// columns of position p leave here, for record p of the lane's ray: its first write to them (the flush opens the record).
template <int EXP, int ERF, int EC, bool RAYS, bool ORDERED>
__device__ __forceinline__ void ray_grad_chunk(const GradSink<ORDERED> &sink, const SceneTables *Sp, const uint32_t *s_list /*[k*64 + lane]*/, float *s_acc,
                                               uint32_t nl, uint32_t nmax, uint32_t lane, const LaneRay &ray, uint32_t i0, float4 g, float &W)
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

    // ---- pass 1: the exponents of T at the chunk's 5 EC sample points (the radiance kernel's pair loop) ----
    float acc[EC][5];
#pragma unroll
    for (int e = 0; e < EC; ++e)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[e][k] = 0.f;
    const LaneList L = { s_list, lane, nl, nmax };
    ListWalk lw = grad_walk_begin(S, L);
    for (uint32_t j = 0; j < nmax; ++j) grad_pass1(erf, grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j), e_mubar, e_sigma, acc);

    // ---- the emitters: w_ik, V_i; the albedo rows leave here ----
    float w[EC][5], GV[EC];
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const bool on = i0 + e < nl;
        const uint32_t idx = on ? s_list[(i0 + e) * 64 + lane] : 0u;
        const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], on, ray);
        const float4 alb = S.gC[idx];
        const float mag = on ? S.gD[idx].z : 0.f;
        const float G = on ? g.x * alb.x + g.y * alb.y + g.z * alb.z + g.w * alb.w : 0.f;
        const float V = grad_emitter<EXP>(on, e_sigma[e], q.d2, 0.5f * q.inv_s2, G * mag, acc[e], w[e]);
        GV[e] = G * V;
        W = __builtin_fmaf(GV[e], mag, W);
        const float mV = mag * V;
        const float da[4] = { g.x * mV, g.y * mV, g.z * mV, g.w * mV };
        if (sink.template wanted<RAYS>()) sink.template deposit<4>((uint64_t)i0 + e, idx, on, da, 0u, lane, GRAD_STORE);
    }

    // ---- pass 2: the same pairs again; w_ik to the absorbers (P, Q, R) and through w e2 A C r back to the emitters (Z, Y) ----
    float z[EC], y[EC];
#pragma unroll
    for (int e = 0; e < EC; ++e) z[e] = y[e] = 0.f;
    lw = grad_walk_begin(S, L);
    for (uint32_t j = 0; j < nmax; ++j) {
        const GradGauss q = grad_walk_next<EXP, ERF>(lw, S, erf, L, ray, j);
        float Pj = 0.f, Qj = 0.f, Rj = 0.f;
        grad_pass2<EXP>(erf, q, e_mubar, e_sigma, w, z, y, Pj, Qj, Rj);
        grad_acc(s_acc, 0, j, lane) += q.Am * Pj;
        grad_acc(s_acc, 1, j, lane) += q.Ar * Qj;
        grad_acc(s_acc, 2, j, lane) += q.Ar * Rj * SQRT_2;
    }
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        if (i0 + e < nl) {
            grad_acc(s_acc, 0, i0 + e, lane) += GV[e];
            grad_acc(s_acc, 1, i0 + e, lane) -= z[e];
            grad_acc(s_acc, 2, i0 + e, lane) -= y[e];
        }
    }
}

// RAYS: the ray rows are asked for (P.grad_rays != nullptr), and then the table may be missing; without, the table is there.
// ORDERED: one record per list position, the lane's own -- the albedo columns at the emitter's chunk, columns 4..8 and the name at the
// flush.  <.., false> is the kernel as it is without.
template <int EXP, int ERF, int SRC, bool RAYS, bool ORDERED = false>
__global__ __launch_bounds__(64) void ray_short_grad_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    __shared__ float s_acc[3 * RAY_PL * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane); // the cull: exactly the radiance kernel's
    const uint32_t nl = R.nl, nmax = R.nmax;
    const LaneRay &ray = R.ray;
    const float4 g = P.grad_radiance[R.rc];
    GradSink<ORDERED> sink(&P, false);
    sink.short_ray(R);

    for (uint32_t p = 0; p < nmax; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c) grad_acc(s_acc, c, p, lane) = 0.f;

    float W = 0.f;
    constexpr int EC = 4;
    for (uint32_t i0 = 0; i0 < nmax; i0 += EC) {
        const uint32_t rem = nmax - i0;
        if (rem >= (uint32_t)EC) ray_grad_chunk<EXP, ERF, EC, RAYS>(sink, &S, s_list, s_acc, nl, nmax, lane, ray, i0, g, W);
        else if (rem == 3) ray_grad_chunk<EXP, ERF, 3, RAYS>(sink, &S, s_list, s_acc, nl, nmax, lane, ray, i0, g, W);
        else if (rem == 2) ray_grad_chunk<EXP, ERF, 2, RAYS>(sink, &S, s_list, s_acc, nl, nmax, lane, ray, i0, g, W);
        else ray_grad_chunk<EXP, ERF, 1, RAYS>(sink, &S, s_list, s_acc, nl, nmax, lane, ray, i0, g, W);
    }

    grad_flush_short<EXP, ERF, RAYS>(sink, P.grad_rays, R.rc, R.writes, S, ErfEval<ERF>(), LaneList{ s_list, lane, nl, nmax }, s_acc, ray, W);
}

// One wave per long ray, lane = emitter (EC rounds of 64 at a time), the absorber wave-uniform.  RAYS: as in the short kernel.  A template
// parameter in all four gradient kernels: with a pointer test the six accumulators cost this one an occupancy step in five of its eight
// instantiations, and the others a fraction of a percent of their time (profiles/ray_grad_rays.md); <.., false> is each kernel as it was.
// ORDERED: two records per kept Gaussian in the ray's range.  The EMITTER record of position p (record p) belongs to the lane that holds p
// as an emitter, lane p mod 64, in its round and again in the last walk: it opens it with the albedo columns, stores the emitter's own
// terms, then adds the W terms onto its own stores.  The ABSORBER record of position j (record n + j) is the wave's (GradSink::absorber),
// its first write in the first round.
template <int EXP, int ERF, int SRC, bool RAYS, bool ORDERED = false>
__global__ __launch_bounds__(64) void ray_long_grad_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    const ErfEval<ERF> erf;
    constexpr int EC = 2;
    GradSink<ORDERED> sink(&P, false);
    const bool table = sink.template wanted<RAYS>(); // wave-uniform

    LongRay L = ray_long_begin<SRC>(&P);
    while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) {
        const LaneRay ray = L.ray;
        const uint32_t n = L.n;
        const float4 g = P.grad_radiance[L.r];
        if (!sink.long_ray(L.r, n, 2u, lane)) continue;
        float W = 0.f; // this lane's emitters; summed over the wave behind the rounds
        [[maybe_unused]] float go[3] = { 0.f, 0.f, 0.f }, gn[3] = { 0.f, 0.f, 0.f }; // this lane's shares of the ray's row; summed over the wave behind the last walk
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
            // ---- the emitters ----
            float w[EC][5], GV[EC], e_mag[EC];
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[e_idx[e]], S.gB[e_idx[e]], e_on[e], ray);
                const float4 alb = S.gC[e_idx[e]];
                e_mag[e] = e_on[e] ? S.gD[e_idx[e]].z : 0.f;
                const float G = e_on[e] ? g.x * alb.x + g.y * alb.y + g.z * alb.z + g.w * alb.w : 0.f;
                const float V = grad_emitter<EXP>(e_on[e], e_sigma[e], q.d2, 0.5f * q.inv_s2, G * e_mag[e], acc[e], w[e]);
                GV[e] = G * V;
                W = __builtin_fmaf(GV[e], e_mag[e], W);
                if (table && e_on[e]) {
                    const float mV = e_mag[e] * V;
                    const float da[4] = { g.x * mV, g.y * mV, g.z * mV, g.w * mV };
                    sink.template put<4>((uint64_t)e0 + (uint32_t)e * 64u + lane, e_idx[e], 0u, da, GRAD_OPEN);
                }
            }
            // ---- pass 2: per absorber P, Q, R over the wave, one row segment by lanes 0..4 ----
            float z[EC], y[EC];
#pragma unroll
            for (int e = 0; e < EC; ++e) z[e] = y[e] = 0.f;
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t idx = __builtin_amdgcn_readfirstlane(long_list_entry(s_list, L.slot, j));
                const GradGauss q = grad_gauss<EXP, ERF>(erf, uload(S.mu_sig, idx), uload(S.gB, idx), true, ray);
                float Pj = 0.f, Qj = 0.f, Rj = 0.f;
                grad_pass2<EXP>(erf, q, e_mubar, e_sigma, w, z, y, Pj, Qj, Rj);
                Pj = wave_sum(Pj); Qj = wave_sum(Qj); Rj = wave_sum(Rj);
                const float mag = uload(S.gD, idx).z;
                if (RAYS && lane == 0) grad_ray_add(q, ray, mag, q.Am * Pj, q.Ar * Qj, go, gn); // wave-uniform: one lane takes it
                if (table) {
                    float d[5];
                    grad_row(q, ray, mag, q.Am * Pj, q.Ar * Qj, q.Ar * Rj * SQRT_2, d);
                    sink.absorber((uint64_t)n + j, idx, lane == 0 ? d[0] : lane == 1 ? d[1] : lane == 2 ? d[2] : lane == 3 ? d[3] : d[4], lane, e0 == 0u);
                }
            }
            // ---- the emitters' own terms: every lane another row ----
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                if (e_on[e]) {
                    const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[e_idx[e]], S.gB[e_idx[e]], true, ray);
                    if constexpr (RAYS) grad_ray_add(q, ray, e_mag[e], GV[e], -z[e], go, gn);
                    if (table) {
                        float d[5];
                        grad_row(q, ray, e_mag[e], GV[e], -z[e], -y[e], d);
                        sink.template put<5>((uint64_t)e0 + (uint32_t)e * 64u + lane, e_idx[e], 4u, d, GRAD_STORE);
                    }
                }
            }
        }
        // ---- the terms in W = sum_ik w_ik, lane = list position ----
        W = wave_sum(W);
        for (uint32_t p0 = 0; p0 < n; p0 += 64u) {
            const uint32_t p = p0 + lane;
            if (p < n) {
                const uint32_t idx = long_list_entry(s_list, L.slot, p);
                const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], true, ray);
                const float ArEW = q.Ar * exp_neg_sq<EXP>(q.m) * W;
                if constexpr (RAYS) grad_ray_add(q, ray, 0.f, 0.f, -ArEW, go, gn);
                if (table) {
                    const float dw[4] = { -ArEW * ray.nx, -ArEW * ray.ny, -ArEW * ray.nz, ArEW * q.m * SQRT_2 };
                    sink.template put<4>(p, idx, 4u, dw, GRAD_STORE, false); // onto this lane's own stores: p mod 64 is its lane in every round
                }
            }
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
static void launch_ray_grad_bundle_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    grad_dispatch_source_rays(src, a.grad_rays != nullptr, [&](auto I, auto R) {
        launch_ray_kernels(ray_short_grad_kernel<EXP, ERF, I.value, R.value, false>, ray_long_grad_kernel<EXP, ERF, I.value, R.value, false>, a, long_grid, st);
    });
}
// the four pairs of VRT_DISPATCH_GRAD_PAIR; out of line here because the entry points' check (vrt_hip_rays.cpp) asks too
bool ray_grad_pair_supported(int exp_kind, int erf_kind)
{
    return (exp_kind == VRT_EXP_VCL || exp_kind == VRT_EXP_LIBM) && (erf_kind == VRT_ERF_AS || erf_kind == VRT_ERF_LIBM);
}
void launch_ray_grad_bundle(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !long_grid || !ray_grad_pair_supported(exp_kind, erf_kind)) return;
    VRT_DISPATCH_GRAD_PAIR(launch_ray_grad_bundle_t, a, long_grid, src, st);
}

#else // vrt_ray_grad_ordered_kernel.hip: the ORDERED instantiations alone, so that the build stays parallel
template <int EXP, int ERF>
static void launch_ray_grad_bundle_ordered_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    grad_dispatch_source_rays(src, a.grad_rays != nullptr, [&](auto I, auto R) {
        launch_ray_kernels(ray_short_grad_kernel<EXP, ERF, I.value, R.value, true>, ray_long_grad_kernel<EXP, ERF, I.value, R.value, true>, a, long_grid, st);
    });
}
void launch_ray_grad_bundle_ordered(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !long_grid || !a.grad || !ray_grad_pair_supported(exp_kind, erf_kind)) return;
    VRT_DISPATCH_GRAD_PAIR(launch_ray_grad_bundle_ordered_t, a, long_grid, src, st);
}
#endif

} // namespace vrtk
