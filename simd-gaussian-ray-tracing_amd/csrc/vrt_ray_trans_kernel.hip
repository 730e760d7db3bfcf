// vrt_ray_trans_kernel.hip -- transmittance bundles (vrt_hip_transmittance_bundle*): T at ns sample distances along caller-given rays,
// broadcast_transmittance (rt.h:102-127) over the Gaussians each ray keeps under the ray bundles' cull rule.  The cull, the queue of the
// long rays, the re-cull and the statistics are vrt_ray_cull.hpp's, the text the radiance kernels of vrt_ray_kernel.hip run: the same
// rays keep the same Gaussians and go to the same kind of kernel.
//   ray_short_trans_kernel  lane = ray, one wave per 64 consecutive rays; per-ray lists of at most RAY_PL scene indices in LDS; a ray's
//                           exponent is transmittance_term added in ascending scene order, the reference's sum without what the cull drops
//   ray_long_trans_kernel   one wave per ray whose list is longer, lane l takes entries l, l + 64, ...; the 64 partial sums are reduced
//                           in a fixed order (wave_sum) -- another summation order than the reference's
// A dropped Gaussian has sigma mag exp(-x) < eps_eff and its term is at most 2 / sqrt(2 pi) times that: the exponent moves by less than
// 0.8 cull_eps min(N, 4096).
// Compiled with the default scheduler: nobody has measured -amdgpu-sched-strategy=max-ilp on these loops.
#include "vrt_ray_trans.hpp" // trans_entry, trans_sample, RAY_SG, long_list_entry: shared with vrt_ray_depth_kernel.hip

namespace vrtk {

template <int EXP, int ERF, bool INDEXED>
__global__ __launch_bounds__(64) void ray_short_trans_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r = (uint64_t)blockIdx.x * 64u + lane;
    const bool valid = r < P.nrays; // the grid has no wave without a valid ray
    const uint64_t rc = valid ? r : P.nrays - 1;
    const LaneRay ray = load_ray(P, rc);

    // ---- cull (vrt_ray_cull.hpp): exactly the radiance kernel's ----
    const uint32_t N = S.n, nch = (N + 63u) / 64u;
    RayCullCounts cnt;
    uint32_t nl = ray_short_cull<INDEXED>(&P, &S, N, nch, s_list, lane, valid, ray, cnt);
    const bool is_long = nl > (uint32_t)RAY_PL;
    ray_short_file<INDEXED>(&P, nch, r, valid, is_long, nl, cnt); // to the one-wave-per-ray kernel behind this one; statistics

    // ---- samples, RAY_SG at a time: every lane walks its own list once per group; the loops run to the longest list of the wave's
    // short rays, and a lane past the end of its list leaves its sums as they are ----
    if (is_long) nl = 0;
    const uint32_t nmax = wave_max_u32(nl);
    const uint64_t ns = P.ns;
    const float *sp = P.s + (P.s_per_ray ? rc * ns : 0ull);
    float *Tp = P.T + rc * ns;
    const bool writes = valid && !is_long;
    for (uint64_t k0 = 0; k0 < ns; k0 += RAY_SG) {
        float sv[RAY_SG], acc[RAY_SG];
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g) {
            sv[g] = k0 + g < ns ? sp[k0 + g] : 0.f;
            acc[g] = 0.f;
        }
        if (nmax) {
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
#pragma unroll
                for (int g = 0; g < RAY_SG; ++g) {
                    const float sum = add_ref(acc[g], trans_sample<ERF>(t, sv[g]));
                    acc[g] = vj ? sum : acc[g];
                }
            }
        }
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g)
            if (writes && k0 + g < ns) Tp[k0 + g] = vexp<EXP>(acc[g]);
    }
}

// One wave per long ray.  Claim, re-cull and list are the radiance long kernel's (vrt_ray_cull.hpp).  Lane l takes entries l, l + 64, ...
// with per-lane gathers of the rows; RAY_SG partial sums per pass over the list are reduced over the lanes in a fixed order.
template <int EXP, int ERF, bool INDEXED>
__global__ __launch_bounds__(64) void ray_long_trans_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_long = min(P.counters[0], P.queue_cap); // final: the short kernel is done
    uint32_t *slot = P.scratch + (size_t)blockIdx.x * S.n;
    const uint32_t N = S.n, nch = (N + 63u) / 64u;
    const uint64_t ns = P.ns;

    while (true) {
        const uint32_t k = ray_long_claim(&P, lane); // every lane executes the atomic: see there
        if (k >= n_long) break;
        const uint64_t r = P.queue[k];
        if (r >= P.nrays) continue;
        const LaneRay ray = load_ray(P, r);

        __syncthreads(); // the previous ray's list reads are done
        const uint32_t n = ray_long_cull<INDEXED>(&P, &S, N, nch, (lds_u32 *)s_list, slot, lane, ray);
        __syncthreads(); // list and scratch writes of this wave are visible to it
        if (P.stats && lane == 0 && n > (uint32_t)RAY_LCAP) atomicAdd(&P.stats[8], 1ull);

        const float *sp = P.s + (P.s_per_ray ? r * ns : 0ull);
        float *Tp = P.T + r * ns;
        for (uint64_t k0 = 0; k0 < ns; k0 += RAY_SG) {
            float sv[RAY_SG], acc[RAY_SG];
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) {
                sv[g] = k0 + g < ns ? sp[k0 + g] : 0.f;
                acc[g] = 0.f;
            }
            for (uint32_t p = lane; p < n; p += 64u) {
                const uint32_t idx = long_list_entry(s_list, slot, p);
                const TransEntry t = trans_entry<EXP, ERF>(S.mu_sig[idx], S.gD[idx].z, ray);
#pragma unroll
                for (int g = 0; g < RAY_SG; ++g) acc[g] = add_ref(acc[g], trans_sample<ERF>(t, sv[g]));
            }
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) {
                const float total = wave_sum(acc[g]); // the whole wave is here again
                if (lane == 0 && k0 + g < ns) Tp[k0 + g] = vexp<EXP>(total);
            }
        }
    }
}

template <int EXP, int ERF>
static void launch_ray_trans_bundle_t(const RayArgs &a, uint32_t long_grid, bool indexed, hipStream_t st)
{
    const dim3 short_grid((uint32_t)((a.nrays + 63u) / 64u));
    if (indexed) {
        hipLaunchKernelGGL((ray_short_trans_kernel<EXP, ERF, true>), short_grid, dim3(64), 0, st, a);
        hipLaunchKernelGGL((ray_long_trans_kernel<EXP, ERF, true>), dim3(long_grid), dim3(64), 0, st, a);
    } else {
        hipLaunchKernelGGL((ray_short_trans_kernel<EXP, ERF, false>), short_grid, dim3(64), 0, st, a);
        hipLaunchKernelGGL((ray_long_trans_kernel<EXP, ERF, false>), dim3(long_grid), dim3(64), 0, st, a);
    }
}
void launch_ray_trans_bundle(const RayArgs &a, uint32_t long_grid, bool indexed, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !a.ns || !long_grid) return;
    VRT_DISPATCH_EXP_ERF(launch_ray_trans_bundle_t, a, long_grid, indexed, st);
}

} // namespace vrtk
