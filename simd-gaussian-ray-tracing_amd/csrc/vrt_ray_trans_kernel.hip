// vrt_ray_trans_kernel.hip -- transmittance bundles (vrt_hip_transmittance_bundle*): T at ns sample distances along caller-given rays,
// broadcast_transmittance (rt.h:102-127) over the Gaussians each ray keeps under the ray bundles' cull rule.  The cull, the queue of the
// long rays, the re-cull and the statistics are vrt_ray_cull.hpp's, the text the radiance kernels of vrt_ray_kernel.hip run: the same
// rays keep the same Gaussians and go to the same kind of kernel.  The walks of the lists are vrt_ray_trans.hpp's, the text the depth
// bundles search.
//   ray_short_trans_kernel  lane = ray, one wave per 64 consecutive rays; per-ray lists of at most RAY_PL scene indices in LDS; a ray's
//                           exponent is transmittance_term added in ascending scene order, the reference's sum without what the cull drops
//   ray_long_trans_kernel   one wave per ray whose list is longer, lane l takes entries l, l + 64, ...; the 64 partial sums are reduced
//                           in a fixed order (wave_sum) -- another summation order than the reference's
// A dropped Gaussian has sigma mag exp(-x) < eps_eff and its term is at most 2 / sqrt(2 pi) times that: the exponent moves by less than
// 0.8 cull_eps min(N, 4096).
// Compiled with the default scheduler: nobody has measured -amdgpu-sched-strategy=max-ilp on these loops.
#include "vrt_ray_trans.hpp" // short_walk, long_walk, RAY_SG: shared with vrt_ray_depth_kernel.hip

namespace vrtk {

template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_short_trans_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    const uint32_t lane = threadIdx.x & 63u;
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane); // the cull: exactly the radiance kernel's

    // ---- samples, RAY_SG at a time: every lane walks its own list once per group ----
    const uint64_t ns = P.ns;
    const float *sp = P.s + (P.s_per_ray ? R.rc * ns : 0ull);
    float *Tp = P.T + R.rc * ns;
    for (uint64_t k0 = 0; k0 < ns; k0 += RAY_SG) {
        float sv[RAY_SG], acc[RAY_SG];
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g) sv[g] = k0 + g < ns ? sp[k0 + g] : 0.f;
        short_walk<EXP, ERF, RAY_SG, false>(&S, s_list, lane, R.nl, R.nmax, R.ray, sv, acc);
#pragma unroll
        for (int g = 0; g < RAY_SG; ++g)
            if (R.writes && k0 + g < ns) Tp[k0 + g] = vexp<EXP>(acc[g]);
    }
}

// One wave per long ray.  Claim, re-cull and list are the radiance long kernel's (vrt_ray_cull.hpp); RAY_SG sums per walk of the list.
template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_long_trans_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ns = P.ns;

    LongRay L = ray_long_begin<SRC>(&P);
    while (ray_long_next<SRC>(&P, &S, s_list, lane, L)) {
        const float *sp = P.s + (P.s_per_ray ? L.r * ns : 0ull);
        float *Tp = P.T + L.r * ns;
        for (uint64_t k0 = 0; k0 < ns; k0 += RAY_SG) {
            float sv[RAY_SG], total[RAY_SG];
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g) sv[g] = k0 + g < ns ? sp[k0 + g] : 0.f;
            long_walk<EXP, ERF, RAY_SG, false>(&S, s_list, L.slot, lane, L.n, L.ray, sv, total);
#pragma unroll
            for (int g = 0; g < RAY_SG; ++g)
                if (lane == 0 && k0 + g < ns) Tp[k0 + g] = vexp<EXP>(total[g]);
        }
    }
}

template <int EXP, int ERF>
static void launch_ray_trans_bundle_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    if (src == RAY_LIST_PLAN) launch_ray_kernels(ray_short_trans_kernel<EXP, ERF, RAY_LIST_PLAN>, ray_long_trans_kernel<EXP, ERF, RAY_LIST_PLAN>, a, long_grid, st);
    else if (src == RAY_LIST_INDEX) launch_ray_kernels(ray_short_trans_kernel<EXP, ERF, RAY_LIST_INDEX>, ray_long_trans_kernel<EXP, ERF, RAY_LIST_INDEX>, a, long_grid, st);
    else launch_ray_kernels(ray_short_trans_kernel<EXP, ERF, RAY_LIST_CHUNKS>, ray_long_trans_kernel<EXP, ERF, RAY_LIST_CHUNKS>, a, long_grid, st);
}
void launch_ray_trans_bundle(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !a.ns || !long_grid) return;
    VRT_DISPATCH_EXP_ERF(launch_ray_trans_bundle_t, a, long_grid, src, st);
}

} // namespace vrtk
