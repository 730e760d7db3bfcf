// vrt_query_kernel.hip -- the point queries: transmittance (at samples of one ray, per ray, and by the reference's Riemann sum), density,
// radiance of arbitrary rays over the whole scene, and the Exp / Erf variants evaluated on their own.
#include "vrt_kernels_common.hpp"

namespace vrtk {

// API parity with rt.h:32-54, rt.cpp:8-27, rt.h:146-223; not performance paths.
// (transmittance_term: vrt_kernels_common.hpp)
template <int EXP, int ERF>
__global__ void transmittance_kernel(SceneTables S, float ox, float oy, float oz, float nx, float ny, float nz,
                                     const float *s_in, size_t ns, float *T_out)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ns) return;
    const float s = s_in[k];
    float T = 0.f;
    for (uint32_t q = 0; q < S.n; ++q) T = add_ref(T, transmittance_term<EXP, ERF>(S, q, ox, oy, oz, nx, ny, nz, s));
    T_out[k] = vexp<EXP>(T);
}
// The same per ray: ray k has its own origin, direction and sample point -- broadcast_transmittance (rt.h:102-127),
// lane = ray.  The arithmetic is transmittance_kernel's (exact divides; the reference's rcp14 estimates are not
// reproduced).
template <int EXP, int ERF>
__global__ void transmittance_rays_kernel(SceneTables S, const float *origins, const float *dirs, const float *s_in,
                                          size_t nrays, float *T_out)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrays) return;
    const float ox = origins[3 * k], oy = origins[3 * k + 1], oz = origins[3 * k + 2];
    const float nx = dirs[3 * k], ny = dirs[3 * k + 1], nz = dirs[3 * k + 2];
    const float s = s_in[k];
    float T = 0.f;
    for (uint32_t q = 0; q < S.n; ++q) T = add_ref(T, transmittance_term<EXP, ERF>(S, q, ox, oy, oz, nx, ny, nz, s));
    T_out[k] = vexp<EXP>(T);
}
template <int EXP, int ERF>
static void launch_transmittance_rays_t(const SceneTables &s, const float *d_o, const float *d_n, const float *d_s, size_t nrays,
                                        float *d_T, hipStream_t st)
{
    hipLaunchKernelGGL((transmittance_rays_kernel<EXP, ERF>), dim3((uint32_t)((nrays + 63) / 64)), dim3(64), 0, st, s, d_o,
                       d_n, d_s, nrays, d_T);
}
void launch_transmittance_rays(const SceneTables &s, const float *d_o, const float *d_n, const float *d_s, size_t nrays,
                               float *d_T, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!nrays) return;
    VRT_DISPATCH_EXP_ERF(launch_transmittance_rays_t, s, d_o, d_n, d_s, nrays, d_T, st);
}

template <int EXP, int ERF>
static void launch_transmittance_t(const SceneTables &s, const float o[3], const float n[3], const float *d_s, size_t ns,
                                   float *d_T, hipStream_t st)
{
    hipLaunchKernelGGL((transmittance_kernel<EXP, ERF>), dim3((uint32_t)((ns + 63) / 64)), dim3(64), 0, st, s, o[0],
                       o[1], o[2], n[0], n[1], n[2], d_s, ns, d_T);
}
void launch_transmittance(const SceneTables &s, const float o[3], const float n[3], const float *d_s, size_t ns,
                          float *d_T, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!ns) return;
    VRT_DISPATCH_EXP_ERF(launch_transmittance_t, s, o, n, d_s, ns, d_T, st);
}

// rt.cpp:8-17: Riemann sum with step delta, fast_exp of the negated sum
__global__ void transmittance_step_kernel(SceneTables S, float ox, float oy, float oz, float nx, float ny, float nz,
                                          const float *s_in, size_t ns, float delta, float *T_out)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ns) return;
    const float s = s_in[k];
    float T = 0.f;
    for (float t = 0; t <= s; t += delta)
        for (uint32_t q = 0; q < S.n; ++q) {
            const float4 g = S.mu_sig[q];
            const float dx = ox + nx * t - g.x, dy = oy + ny * t - g.y, dz = oz + nz * t - g.z;
            T += delta * (S.gD[q].z * exp_accurate(-(dx * dx + dy * dy + dz * dz) / (2 * g.w * g.w)));
        }
    T_out[k] = exp_fast(-T);
}
void launch_transmittance_step(const SceneTables &s, const float o[3], const float n[3], const float *d_s, size_t ns,
                               float delta, float *d_T, hipStream_t st)
{
    if (!ns) return;
    hipLaunchKernelGGL(transmittance_step_kernel, dim3((uint32_t)((ns + 63) / 64)), dim3(64), 0, st, s, o[0], o[1],
                       o[2], n[0], n[1], n[2], d_s, ns, delta, d_T);
}

// rt.cpp:19-27
__global__ void density_kernel(SceneTables S, const float *pts, size_t npts, float *D)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npts) return;
    const float x = pts[3 * k], y = pts[3 * k + 1], z = pts[3 * k + 2];
    float acc = 0.f;
    for (uint32_t q = 0; q < S.n; ++q) {
        const float4 g = S.mu_sig[q];
        const float dx = x - g.x, dy = y - g.y, dz = z - g.z;
        acc += S.gD[q].z * exp_accurate(-(dx * dx + dy * dy + dz * dz) / (2 * g.w * g.w));
    }
    D[k] = acc;
}
void launch_density(const SceneTables &s, const float *d_pts, size_t npts, float *d_D, hipStream_t st)
{
    if (!npts) return;
    hipLaunchKernelGGL(density_kernel, dim3((uint32_t)((npts + 63) / 64)), dim3(64), 0, st, s, d_pts, npts, d_D);
}

// arbitrary rays: lane = ray, every Gaussian of the scene, per-lane origin
template <int EXP, int ERF>
__global__ __launch_bounds__(64) void radiance_kernel(SceneTables S, const float *origins, const float *dirs,
                                                       size_t nrays, const uint32_t *iota, float4 *out)
{
    const size_t r = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t rc = r < nrays ? r : nrays - 1;
    LaneRay ray;
    ray.ox = origins[3 * rc]; ray.oy = origins[3 * rc + 1]; ray.oz = origins[3 * rc + 2];
    ray.nx = dirs[3 * rc]; ray.ny = dirs[3 * rc + 1]; ray.nz = dirs[3 * rc + 2];
    float Lr, Lg, Lb, La;
    shade_list<EXP, ERF, 4, false>(S, iota, S.n, ray, Lr, Lg, Lb, La);
    if (r < nrays) out[r] = make_float4(Lr, Lg, Lb, La);
}
template <int EXP, int ERF>
static void launch_radiance_t(const SceneTables &s, const float *d_origins, const float *d_dirs, size_t nrays,
                              const uint32_t *iota, float4 *d_out, hipStream_t st)
{
    hipLaunchKernelGGL((radiance_kernel<EXP, ERF>), dim3((uint32_t)((nrays + 63) / 64)), dim3(64), 0, st, s, d_origins,
                       d_dirs, nrays, iota, d_out);
}
void launch_radiance(const SceneTables &s, const float *d_origins, const float *d_dirs, size_t nrays,
                     const uint32_t *iota, float4 *d_out, int exp_kind, int erf_kind, hipStream_t st)
{
    if (!nrays) return;
    VRT_DISPATCH_EXP_ERF(launch_radiance_t, s, d_origins, d_dirs, nrays, iota, d_out, st);
}

template <int K>
__global__ void eval_erf_kernel(const float *x, size_t n, float *y)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = verf<K>(x[i]);
}
template <int K>
__global__ void eval_exp_kernel(const float *x, size_t n, float *y)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = vexp<K>(x[i]);
}
void launch_eval_erf(int kind, const float *x, size_t n, float *y, hipStream_t st)
{
    if (!n) return;
    const dim3 g((uint32_t)((n + 255) / 256)), b(256);
    switch (kind) {
    case VRT_ERF_AS: hipLaunchKernelGGL(eval_erf_kernel<VRT_ERF_AS>, g, b, 0, st, x, n, y); break;
    case VRT_ERF_SPLINE: hipLaunchKernelGGL(eval_erf_kernel<VRT_ERF_SPLINE>, g, b, 0, st, x, n, y); break;
    case VRT_ERF_SPLINE_MIRROR: hipLaunchKernelGGL(eval_erf_kernel<VRT_ERF_SPLINE_MIRROR>, g, b, 0, st, x, n, y); break;
    case VRT_ERF_TAYLOR: hipLaunchKernelGGL(eval_erf_kernel<VRT_ERF_TAYLOR>, g, b, 0, st, x, n, y); break;
    default: hipLaunchKernelGGL(eval_erf_kernel<VRT_ERF_LIBM>, g, b, 0, st, x, n, y); break;
    }
}
void launch_eval_exp(int kind, const float *x, size_t n, float *y, hipStream_t st)
{
    if (!n) return;
    const dim3 g((uint32_t)((n + 255) / 256)), b(256);
    switch (kind) {
    case VRT_EXP_VCL: hipLaunchKernelGGL(eval_exp_kernel<VRT_EXP_VCL>, g, b, 0, st, x, n, y); break;
    case VRT_EXP_FAST: hipLaunchKernelGGL(eval_exp_kernel<VRT_EXP_FAST>, g, b, 0, st, x, n, y); break;
    case VRT_EXP_SPLINE: hipLaunchKernelGGL(eval_exp_kernel<VRT_EXP_SPLINE>, g, b, 0, st, x, n, y); break;
    default: hipLaunchKernelGGL(eval_exp_kernel<VRT_EXP_LIBM>, g, b, 0, st, x, n, y); break;
    }
}
} // namespace vrtk
