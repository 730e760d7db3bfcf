// vrt_hip_rays.cpp -- ray bundles of libvrt_hip.so (vrt_hip_radiance_rays*): radiance of caller-given rays, culled per ray
// (vrt_ray_kernel.hip).  The scene tables and the chunk spheres are the frame pipeline's; the long-ray queue, its counters and the
// long kernel's scratch slots belong to the context and only grow.
#include <algorithm>

#include "vrt_hip_ctx.hpp"

using namespace vrtk;

namespace {

// One-wave workgroups of the long kernel: four per CU, fewer for scenes whose scratch slots (N words each) would pass 256 MB.
// A function of the scene size alone; which kernel shades a ray never depends on it.
uint32_t long_grid(const vrt_hip_ctx *c)
{
    const uint64_t by_memory = ((uint64_t)64 << 20) / std::max<uint64_t>(c->n, 1);
    return (uint32_t)std::max<uint64_t>(16, std::min<uint64_t>((uint64_t)c->num_cus * 4, by_memory));
}

} // namespace

extern "C" {

int vrt_hip_radiance_rays_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                 float *d_radiance, uint32_t *d_image, int pack_flags, void *hip_stream)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (nrays == 0) return VRT_HIP_OK;
    if (!d_origins || !d_dirs) return fail(c, VRT_HIP_ERR_INVALID, "radiance_rays: NULL origins or directions");
    if (!d_radiance && !d_image) return fail(c, VRT_HIP_ERR_INVALID, "radiance_rays: no output buffer");
    if (nrays > 0xFFFFFFF0ull) return fail(c, VRT_HIP_ERR_INVALID, "radiance_rays: more than 2^32 - 16 rays in one bundle");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    { int rc = rebuild_tables(c); if (rc) return rc; }
    wait_for_last_stream(c, st); // a bundle in flight on another stream uses the queue and the scratch slots
    c->last_stream = st;
    const uint32_t grid = long_grid(c);
    // (a buffer that grows is freed first, which waits for the device: no bundle in flight loses its memory)
    HIPCHK(c, c->ray_queue.reserve(nrays));
    HIPCHK(c, c->ray_counters.reserve(2));
    HIPCHK(c, c->ray_scratch.reserve((size_t)grid * c->n));
    HIPCHK(c, c->ray_stats.reserve(RAY_STATS_WORDS));
    HIPCHK(c, hipMemsetAsync(c->ray_counters.p, 0, 2 * sizeof(uint32_t), st));
    if (c->stats_on) HIPCHK(c, hipMemsetAsync(c->ray_stats.p, 0, RAY_STATS_WORDS * sizeof(unsigned long long), st));
    c->ray_stats_valid = c->stats_on;
    RayArgs a{};
    a.S = tables(c);
    a.chunks = c->gChunk.p;
    a.origins = d_origins; a.dirs = d_dirs; a.origin_per_ray = origin_per_ray ? 1 : 0;
    a.nrays = nrays;
    a.radiance = (float4 *)d_radiance; a.image = d_image; a.pack_flags = pack_flags;
    a.queue = c->ray_queue.p; a.queue_cap = (uint32_t)nrays;
    a.counters = c->ray_counters.p;
    a.scratch = c->ray_scratch.p;
    a.stats = c->stats_on ? c->ray_stats.p : nullptr;
    launch_ray_bundle(a, grid, c->exp_kind, c->erf_kind, st);
    HIPCHK(c, hipGetLastError());
    return VRT_HIP_OK;
}

int vrt_hip_radiance_rays(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                          float *radiance_out, uint32_t *image_out, int pack_flags)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (nrays == 0) return VRT_HIP_OK;
    if (!origins || !dirs) return fail(c, VRT_HIP_ERR_INVALID, "radiance_rays: NULL origins or directions");
    if (!radiance_out && !image_out) return fail(c, VRT_HIP_ERR_INVALID, "radiance_rays: no output buffer");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // the staging buffers may still be read by an earlier bundle
    const size_t no = (origin_per_ray ? nrays : 1) * 3;
    HIPCHK(c, c->rays_in[0].reserve(no));
    HIPCHK(c, c->rays_in[1].reserve(nrays * 3));
    if (radiance_out) HIPCHK(c, c->rays_rad.reserve(nrays));
    if (image_out) HIPCHK(c, c->rays_img.reserve(nrays));
    HIPCHK(c, hipMemcpyAsync(c->rays_in[0].p, origins, no * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rays_in[1].p, dirs, nrays * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    int rc = vrt_hip_radiance_rays_device(c, nrays, c->rays_in[0].p, origin_per_ray, c->rays_in[1].p, radiance_out ? (float *)c->rays_rad.p : nullptr,
                                          image_out ? c->rays_img.p : nullptr, pack_flags, c->stream);
    if (rc) return rc;
    if (radiance_out) HIPCHK(c, hipMemcpyAsync(radiance_out, c->rays_rad.p, nrays * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (image_out) HIPCHK(c, hipMemcpyAsync(image_out, c->rays_img.p, nrays * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VRT_HIP_OK;
}

int vrt_hip_get_ray_stats(vrt_hip_ctx *c, vrt_hip_ray_stats *out)
{
    if (!c || !out) return VRT_HIP_ERR_INVALID;
    *out = vrt_hip_ray_stats{};
    if (!c->ray_stats_valid) return VRT_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // waits for the bundle
    unsigned long long w[RAY_STATS_WORDS];
    HIPCHK(c, hipMemcpy(w, c->ray_stats.p, sizeof(w), hipMemcpyDeviceToHost));
    out->rays = w[0]; out->short_rays = w[1]; out->long_rays = w[2]; out->lane_entries = w[3]; out->lane_pairs = w[4];
    out->chunks_tested = w[5]; out->chunks_kept = w[6]; out->members_tested = w[7]; out->scratch_rays = w[8];
    return VRT_HIP_OK;
}

} // extern "C"
