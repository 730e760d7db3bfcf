// vrt_ray_kernel.hip -- ray bundles (vrt_hip_radiance_rays*): radiance of caller-given rays, each with its own origin and
// direction, culled per ray like the image kernels' last level.  No camera, no tiles, no cones: the whole scene enters ONE
// level with the tile level's threshold (gB.w), so a ray loses less than 3 * cull_eps * min(N, 4096).
// Two kernels per call, both always enqueued:
//   ray_short_kernel  lane = ray, one wave per 64 consecutive rays; per-ray lists of at most RAY_PL global indices in LDS
//   ray_long_kernel   one wave per ray whose list is longer, lane = emitter; reads its work count on the device
// Which kernel shades a ray depends on that ray's own list length alone, and a lane's list on its own tests alone: a ray's
// bits are a function of (ray, scene, options), whatever its wave-mates are.
// Both kernels come in a second, INDEXED form (vrt_hip_set_ray_index): the cull walks the scene in the Morton order of its centres --
// group spheres (64 leaves), leaf spheres (64 consecutive Morton positions), members -- and hands the shading code the SAME list in
// the same ascending scene order: the sphere tests only ever drop what the member test drops, so no bit of a result moves.
// And in a third, PLANNED form (vrt_hip_set_ray_plan, SRC = RAY_LIST_PLAN): no cull at all, the lists a ray plan kept of this cull.
// What a lane = ray kernel does before it shades (ray, cull, list, filing: ray_short_begin) and how the pair is launched
// (launch_ray_kernels) is vrt_ray_cull.hpp's, the text the transmittance and depth bundles run.  ray_long_kernel keeps its OWN text of
// the claim loop (ray_long_next there), of the list entry (long_list_entry there) and of the emitter set-up and emission it has in common
// with ray_shade_chunk: under max-ilp each of the shared forms moved its pair loop's schedule, and the build with them was slower on
// the bundle that lives in this kernel (profiles/ray_bundle_refactor.md).  A change to ray_long_next is a change to that loop as well.
// Compiled like the block kernel with -mllvm -amdgpu-sched-strategy=max-ilp (see the note at the top of vrt_block_kernel.hip):
// the pair loops are the same independent erf terms.
#include "vrt_ray_cull.hpp"

namespace vrtk {

// Group spheres of the Morton index: lane = leaf sphere of the group, one wave per group.  Centre = mid-point of the box of the leaf
// centres, radius = the farthest leaf centre plus that leaf's radius, widened by build_chunks_kernel's margins: a line farther from the
// centre than that is farther from every leaf centre than the leaf's radius (the distance to a line is 1-Lipschitz in the point).
// A leaf sphere that is not finite (a NaN or infinite centre or reach among its members) makes the radius NaN, which ray_chunk_keeps keeps.
__global__ __launch_bounds__(256) void build_ray_groups_kernel(uint32_t nleaves, const float4 *__restrict__ leaves, float4 *__restrict__ groups)
{
    const uint32_t lane = threadIdx.x & 63u, group = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (group * 64u >= nleaves) return;
    const uint32_t i = group * 64u + lane;
    const bool valid = i < nleaves;
    const float4 p = valid ? leaves[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY && fabsf(p.w) < INFINITY;
    const bool all_finite = __ballot(valid && !finite) == 0ull;
    const float lo_x = wave_min(valid ? p.x : INFINITY), hi_x = wave_max(valid ? p.x : -INFINITY);
    const float lo_y = wave_min(valid ? p.y : INFINITY), hi_y = wave_max(valid ? p.y : -INFINITY);
    const float lo_z = wave_min(valid ? p.z : INFINITY), hi_z = wave_max(valid ? p.z : -INFINITY);
    const float mx = 0.5f * (lo_x + hi_x), my = 0.5f * (lo_y + hi_y), mz = 0.5f * (lo_z + hi_z);
    const float dx = p.x - mx, dy = p.y - my, dz = p.z - mz;
    float rho = wave_max(valid ? sqrtf(dx * dx + dy * dy + dz * dz) + p.w : 0.f);
    rho = rho * 1.0001f + 1e-6f * (1.f + fabsf(mx) + fabsf(my) + fabsf(mz));
    if (lane == 0) groups[group] = make_float4(mx, my, mz, all_finite ? rho : __builtin_nanf(""));
}
void launch_build_ray_groups(uint32_t nleaves, const float4 *leaves, float4 *groups, hipStream_t st)
{
    const uint32_t ngr = (nleaves + 63u) / 64u;
    if (ngr) hipLaunchKernelGGL(build_ray_groups_kernel, dim3((ngr + 3u) / 4u), dim3(256), 0, st, nleaves, leaves, groups);
}

__device__ __forceinline__ void store_ray(const RayArgs &P, uint64_t r, float Lr, float Lg, float Lb, float La)
{
    if (P.image) P.image[r] = pack_pixel(Lr, Lg, Lb, La, P.pack_flags);
    if (P.radiance) P.radiance[r] = make_float4(Lr, Lg, Lb, La);
}

// One chunk of EC emitters (list positions i0 .. i0+EC-1 of every lane) against the lane's whole list: shade_chunk of the block
// kernel with the parameter rows gathered per lane from the scene tables (L2-resident; a coherent bundle reads one address in
// all lanes) and oc = mu - o formed per lane, as shade_list<.., false> does.  The next absorber's rows are fetched one iteration ahead.
template <int EXP, int ERF, int EC>
__device__ __forceinline__ void ray_shade_chunk(const SceneTables &S, const uint32_t *s_list /*[k*64 + lane]*/, uint32_t nl,
                                                uint32_t nmax, uint32_t lane, const LaneRay &ray, uint32_t i0, float &Lr,
                                                float &Lg, float &Lb, float &La)
{
    const ErfEval<ERF> erf;
    float e_mubar[EC], e_sigma[EC];
    uint32_t e_idx[EC];
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        e_idx[e] = (i0 + e < nl) ? s_list[(i0 + e) * 64 + lane] : 0u;
        const float4 ms = S.mu_sig[e_idx[e]];
        const float cx = ms.x - ray.ox, cy = ms.y - ray.oy, cz = ms.z - ray.oz;
        e_mubar[e] = dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz);
        e_sigma[e] = ms.w;
    }
    float acc[EC][5];
#pragma unroll
    for (int e = 0; e < EC; ++e)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[e][k] = 0.f;

    uint32_t lj = nl ? s_list[lane] : 0u;
    float4 a = S.mu_sig[lj], b = S.gB[lj];
    for (uint32_t j = 0; j < nmax; ++j) {
        const float4 ca = a, cb = b;
        const bool vj = j < nl;
        if (j + 1 < nmax) {
            lj = (j + 1 < nl) ? s_list[(j + 1) * 64 + lane] : 0u;
            a = S.mu_sig[lj]; b = S.gB[lj];
        }
        const float cx = ca.x - ray.ox, cy = ca.y - ray.oy, cz = ca.z - ray.oz;
        const float mubar = dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz);
        const float d2 = sub_ref(dot3_ref(cx, cy, cz, cx, cy, cz), mul_ref(mubar, mubar));
        const float A = vj ? cb.z * vexp<EXP>(-(d2 * cb.y)) : 0.f; // past the end of the lane's list: exact zeros
        const float m = mubar * cb.x;
        const float E = erf(-m);
#pragma unroll
        for (int e = 0; e < EC; ++e) {
            const float base = __builtin_fmaf(e_mubar[e], cb.x, -m);
            const float step = e_sigma[e] * cb.x;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const float x = __builtin_fmaf((float)(k - 4), step, base);
                acc[e][k] = __builtin_fmaf(A, E - erf(x), acc[e][k]);
            }
        }
    }

    // emission from the sample point (see shade_list)
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        if (i0 + e < nl) {
            const float4 ms = S.mu_sig[e_idx[e]];
            const float inv2s2 = S.gB[e_idx[e]].y;
            const float q = S.gD[e_idx[e]].y;
            float inner = 0.f;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const float sk = madd_ref((float)(k - 4), ms.w, e_mubar[e]);
                const float px = sub_ref(madd_ref(ray.nx, sk, ray.ox), ms.x);
                const float py = sub_ref(madd_ref(ray.ny, sk, ray.oy), ms.y);
                const float pz = sub_ref(madd_ref(ray.nz, sk, ray.oz), ms.z);
                const float dd = dot3_ref(px, py, pz, px, py, pz);
                inner += emission_term<EXP>(q, dd * inv2s2, acc[e][k]);
            }
            const float4 alb = S.gC[e_idx[e]];
            Lr = __builtin_fmaf(alb.x, inner, Lr);
            Lg = __builtin_fmaf(alb.y, inner, Lg);
            Lb = __builtin_fmaf(alb.z, inner, Lb);
            La = __builtin_fmaf(alb.w, inner, La);
        }
    }
}

template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_short_kernel(RayArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_PL * 64]; // [k*64 + lane]: consecutive lanes on consecutive banks
    const uint32_t lane = threadIdx.x & 63u;
    // ---- ray, cull, list (vrt_ray_cull.hpp) ----
    const ShortRay R = ray_short_begin<SRC>(&P, &S, s_list, lane);
    const uint32_t nl = R.nl, nmax = R.nmax;
    const LaneRay &ray = R.ray;

    // ---- shade: every lane walks its own list; the loops run to the longest list of the wave's short rays ----
    float Lr = 0.f, Lg = 0.f, Lb = 0.f, La = 0.f;
    constexpr int EC = 4;
    for (uint32_t i0 = 0; i0 < nmax; i0 += EC) {
        const uint32_t rem = nmax - i0;
        if (rem >= (uint32_t)EC) ray_shade_chunk<EXP, ERF, EC>(S, s_list, nl, nmax, lane, ray, i0, Lr, Lg, Lb, La);
        else if (rem == 3) ray_shade_chunk<EXP, ERF, 3>(S, s_list, nl, nmax, lane, ray, i0, Lr, Lg, Lb, La);
        else if (rem == 2) ray_shade_chunk<EXP, ERF, 2>(S, s_list, nl, nmax, lane, ray, i0, Lr, Lg, Lb, La);
        else ray_shade_chunk<EXP, ERF, 1>(S, s_list, nl, nmax, lane, ray, i0, Lr, Lg, Lb, La);
    }
    if (R.writes) store_ray(P, R.r, Lr, Lg, Lb, La);
}

// One wave per long ray, lane = emitter.  The ray is wave-uniform: its survivors are compacted in index order (ballot / mbcnt, as the
// block cull does) into s_list, and beyond RAY_LCAP into this workgroup's scratch slot of N words (entry k at slot[k]), so no
// list length is refused.  Lane l then takes emitters l, l + 64, ... against all survivors as absorbers (wave-uniform: scalar
// row loads); the four sums are reduced over the lanes in a fixed order -- another summation order than the reference's.
// INDEXED: the re-cull goes through the Morton index (lane = group, lane = leaf of a kept group, lane = member of a kept leaf) and finds
// the survivors in Morton order; each sets bit perm[pos] of this workgroup's bitmap (N bits of device memory, all zero between rays),
// and the list is read off the bitmap in ascending scene order -- the list the unindexed compaction makes.
template <int EXP, int ERF, int SRC>
__global__ __launch_bounds__(64) void ray_long_kernel(RayArgs)
{
    const RayArgs &P = kernel_args<RayArgs>();
    const SceneTables &S = P.S;
    __shared__ uint32_t s_list[RAY_LCAP];
    const uint32_t lane = threadIdx.x & 63u;
    // RAY_LIST_PLAN (vrt_hip_set_ray_plan): the queue and every list are the plan's, as in ray_long_begin / ray_long_next
    constexpr bool PLANNED = SRC == RAY_LIST_PLAN;
    const uint32_t n_long = PLANNED ? P.pl_nlong : min(P.counters[0], P.queue_cap); // final: the short kernel is done
    uint32_t *slot = PLANNED ? nullptr : P.scratch + (size_t)blockIdx.x * S.n;
    [[maybe_unused]] const uint32_t N = S.n, nch = (N + 63u) / 64u;
    const ErfEval<ERF> erf;
    constexpr int EC = 2;

    while (true) {
        const uint32_t k = ray_long_claim(&P, lane); // every lane executes the atomic: see there
        if (k >= n_long) break;
        uint64_t r;
        if constexpr (PLANNED) r = P.pl_long[k];
        else r = P.queue[k];
        if (r >= P.nrays) continue;
        const LaneRay ray = load_ray(P, r);

        // ---- cull: 64 chunk spheres at a time (lane = chunk), then the members of the kept ones (lane = Gaussian) ----
        __syncthreads(); // the previous ray's list reads are done
        uint32_t n;
        if constexpr (PLANNED) { // ---- or no cull: the first RAY_LCAP entries of the plan's list to LDS, the rest read where they stand ----
            slot = const_cast<uint32_t *>(P.pl_entries + P.pl_off[r]);
            n = min(P.pl_len[r], N);
            for (uint32_t p = lane; p < min(n, (uint32_t)RAY_LCAP); p += 64u) s_list[p] = slot[p];
        } else n = ray_long_cull<SRC>(&P, &S, N, nch, (lds_u32 *)s_list, slot, lane, ray);
        __syncthreads(); // list and scratch writes of this wave are visible to it
        if (P.stats && lane == 0 && n > (uint32_t)RAY_LCAP) atomicAdd(&P.stats[8], 1ull);
        auto entry = [&](uint32_t p) -> uint32_t { return p < (uint32_t)RAY_LCAP ? s_list[p] : slot[p]; };

        // ---- shade ----
        float Lr = 0.f, Lg = 0.f, Lb = 0.f, La = 0.f;
        for (uint32_t e0 = 0; e0 < n; e0 += 64u * EC) {
            float e_mubar[EC], e_sigma[EC];
            uint32_t e_idx[EC];
            bool e_on[EC];
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                const uint32_t p = e0 + (uint32_t)e * 64u + lane;
                e_on[e] = p < n;
                e_idx[e] = entry(e_on[e] ? p : 0u);
                const float4 ms = S.mu_sig[e_idx[e]];
                const float cx = ms.x - ray.ox, cy = ms.y - ray.oy, cz = ms.z - ray.oz;
                e_mubar[e] = dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz);
                e_sigma[e] = ms.w;
            }
            float acc[EC][5];
#pragma unroll
            for (int e = 0; e < EC; ++e)
#pragma unroll
                for (int kk = 0; kk < 5; ++kk) acc[e][kk] = 0.f;
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t idx = __builtin_amdgcn_readfirstlane(entry(j));
                const float4 ms = uload(S.mu_sig, idx), b = uload(S.gB, idx);
                const float cx = ms.x - ray.ox, cy = ms.y - ray.oy, cz = ms.z - ray.oz;
                const float mubar = dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz);
                const float d2 = sub_ref(dot3_ref(cx, cy, cz, cx, cy, cz), mul_ref(mubar, mubar));
                const float A = b.z * vexp<EXP>(-(d2 * b.y));
                const float m = mubar * b.x;
                const float E = erf(-m);
#pragma unroll
                for (int e = 0; e < EC; ++e) {
                    const float base = __builtin_fmaf(e_mubar[e], b.x, -m);
                    const float step = e_sigma[e] * b.x;
#pragma unroll
                    for (int kk = 0; kk < 5; ++kk) {
                        const float x = __builtin_fmaf((float)(kk - 4), step, base);
                        acc[e][kk] = __builtin_fmaf(A, E - erf(x), acc[e][kk]);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                if (e_on[e]) {
                    const float4 ms = S.mu_sig[e_idx[e]];
                    const float inv2s2 = S.gB[e_idx[e]].y;
                    const float q = S.gD[e_idx[e]].y;
                    float inner = 0.f;
#pragma unroll
                    for (int kk = 0; kk < 5; ++kk) {
                        const float sk = madd_ref((float)(kk - 4), ms.w, e_mubar[e]);
                        const float px = sub_ref(madd_ref(ray.nx, sk, ray.ox), ms.x);
                        const float py = sub_ref(madd_ref(ray.ny, sk, ray.oy), ms.y);
                        const float pz = sub_ref(madd_ref(ray.nz, sk, ray.oz), ms.z);
                        const float dd = dot3_ref(px, py, pz, px, py, pz);
                        inner += emission_term<EXP>(q, dd * inv2s2, acc[e][kk]);
                    }
                    const float4 alb = S.gC[e_idx[e]];
                    Lr = __builtin_fmaf(alb.x, inner, Lr);
                    Lg = __builtin_fmaf(alb.y, inner, Lg);
                    Lb = __builtin_fmaf(alb.z, inner, Lb);
                    La = __builtin_fmaf(alb.w, inner, La);
                }
            }
        }
        Lr = wave_sum(Lr); Lg = wave_sum(Lg); Lb = wave_sum(Lb); La = wave_sum(La);
        if (lane == 0) store_ray(P, r, Lr, Lg, Lb, La);
    }
}

template <int EXP, int ERF>
static void launch_ray_bundle_t(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st)
{
    if (src == RAY_LIST_PLAN) launch_ray_kernels(ray_short_kernel<EXP, ERF, RAY_LIST_PLAN>, ray_long_kernel<EXP, ERF, RAY_LIST_PLAN>, a, long_grid, st);
    else if (src == RAY_LIST_INDEX) launch_ray_kernels(ray_short_kernel<EXP, ERF, RAY_LIST_INDEX>, ray_long_kernel<EXP, ERF, RAY_LIST_INDEX>, a, long_grid, st);
    else launch_ray_kernels(ray_short_kernel<EXP, ERF, RAY_LIST_CHUNKS>, ray_long_kernel<EXP, ERF, RAY_LIST_CHUNKS>, a, long_grid, st);
}
void launch_ray_bundle(const RayArgs &a, uint32_t long_grid, int src, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!a.nrays || !long_grid) return;
    VRT_DISPATCH_EXP_ERF(launch_ray_bundle_t, a, long_grid, src, st);
}

} // namespace vrtk
