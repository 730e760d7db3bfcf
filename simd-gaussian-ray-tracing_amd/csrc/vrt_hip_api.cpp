// vrt_hip_api.cpp -- the C ABI of libvrt_hip.so (see include/vrt_hip.h): context, setters, device-resident scene / tile / ray
// state, shard map and static tables.  The frame pipeline over them is vrt_hip_frame.cpp.  Compiled with hipcc for gfx950;
// links only libamdhip64.  There is no CPU fallback anywhere in this file: without a GPU vrt_hip_create() fails.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vrt_hip_ctx.hpp"

using namespace vrtk;

static std::string g_create_error;

int fail(vrt_hip_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// Before work on `st` rewrites what the last frame's kernels on another stream may still be reading, wait for that stream.
// An error from it (it may have been destroyed, which completes its work) is not this call's error.
void wait_for_last_stream(vrt_hip_ctx *c, hipStream_t st)
{
    if (c->last_stream == VRT_NO_STREAM || c->last_stream == st) return;
    if (hipStreamSynchronize(c->last_stream) != hipSuccess) (void)hipGetLastError();
    c->last_stream = st;
}

// Frames enqueued through the *_device entry points run on the CALLER's stream and read the context's tables, lists
// and plane arrays.  Every call that rewrites one of those waits here first -- for the context's own stream and for the
// stream of the last enqueued frame -- so a caller may change state right after enqueueing frames without a
// synchronisation of its own (include/vrt_hip.h, "Streams").
int quiesce(vrt_hip_ctx *c)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    wait_for_last_stream(c, c->stream);
    c->last_stream = VRT_NO_STREAM;
    return VRT_HIP_OK;
}

float exp_floor_x(int exp_kind)
{
    // Exp(-x) is exactly 0 past this point for the chosen Exp, so such Gaussians contribute nothing:
    // vcl_exp flushes below -87.3 (vectormath_exp.h:393); expf reaches 0 below ~-103.98.
    switch (exp_kind) {
    case VRT_EXP_VCL: return 87.3f;
    case VRT_EXP_LIBM: return 104.f;
    case VRT_EXP_FAST: return 88.f;   // clamped fast_exp returns 0 for x < -87.3 (a*x+b < 2^23)
    case VRT_EXP_SPLINE: return 9.0f; // spline_exp(x) = 0 for x <= -9 (approx.cpp:143)
    default: return INFINITY;
    }
}

// table mode applies to the Exp / Erf pairs its error bound covers (vrt_table_kernel.hip, VRT_DISPATCH_TABLE)
bool table_on(const vrt_hip_ctx *c)
{
    return c->table_hx > 0.f && (c->erf_kind == VRT_ERF_AS || c->erf_kind == VRT_ERF_LIBM) &&
           (c->exp_kind == VRT_EXP_VCL || c->exp_kind == VRT_EXP_LIBM);
}

int rebuild_tables(vrt_hip_ctx *c)
{
    if (!c->tables_dirty) return VRT_HIP_OK;
    { int rc = quiesce(c); if (rc) return rc; } // frames in flight read the tables this rewrites
    HIPCHK(c, c->mu_sig.reserve(c->n)); HIPCHK(c, c->gA.reserve(c->n)); HIPCHK(c, c->gB.reserve(c->n));
    HIPCHK(c, c->gC.reserve(c->n)); HIPCHK(c, c->gD.reserve(c->n)); HIPCHK(c, c->iota.reserve(c->n));
    // cull_eps bounds what ONE Gaussian dropped at the tile level could have contributed; a ray can lose all N of them, so
    // for scenes beyond 4096 Gaussians the threshold shrinks with N: 3 * eps_eff * N stays at the 1.2e-5 of N = 4096 and the
    // frame's worst case at 2.5e-5 whatever N is (the lower levels already scale with their list lengths)
    const float eps_eff = c->cull_eps * std::min(1.f, 4096.f / (float)std::max(c->n, 1u));
    launch_build_static(c->n, c->soa[0].p, c->soa[1].p, c->soa[2].p, c->soa[3].p, c->soa[4].p, c->soa[5].p,
                        c->has_alpha ? c->soa[6].p : nullptr, c->soa[7].p, c->soa[8].p, eps_eff,
                        exp_floor_x(c->exp_kind), c->mu_sig.p, c->gB.p, c->gC.p, c->gD.p, c->stream);
    HIPCHK(c, c->gChunk.reserve((c->n + 63u) / 64u));
    launch_build_chunks(c->n, c->mu_sig.p, c->gB.p, c->gChunk.p, c->stream);
    launch_iota(c->iota.p, c->n, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream)); // later launches may use a caller's stream
    c->ray_index_dirty = true;
    if (c->ray_index) { int rc = build_ray_index(c); if (rc) return rc; }
    c->tables_dirty = false;
    c->gA_valid = false;
    c->lists_dirty = true;
    return VRT_HIP_OK;
}

// albedo_scale of a scene set from device memory: one word, read once behind the event recorded at that update
int resolve_albedo_scale(vrt_hip_ctx *c)
{
    if (!c->albedo_pending) return VRT_HIP_OK;
    HIPCHK(c, hipEventSynchronize(c->scene_done));
    uint32_t bits = 0;
    HIPCHK(c, hipMemcpy(&bits, c->scene_words.p + 6, sizeof bits, hipMemcpyDeviceToHost));
    float v;
    memcpy(&v, &bits, sizeof v);
    c->albedo_scale = std::max(1.f, v);
    c->albedo_pending = false;
    return VRT_HIP_OK;
}

SceneTables tables(const vrt_hip_ctx *c)
{
    SceneTables s;
    s.mu_sig = c->mu_sig.p; s.gA = c->gA.p; s.gB = c->gB.p; s.gC = c->gC.p; s.gD = c->gD.p; s.n = c->n;
    return s;
}

// tile geometry for the current image size (rt.h:348-349, 364-365); list pointers filled by the caller
TileLists tile_geometry(const vrt_hip_ctx *c)
{
    TileLists t{};
    if (c->tile_mode != TILES_NONE) {
        t.tiles_w = c->tiles_w; t.tiles_h = c->tiles_h;
        t.tile_w = (uint32_t)(uint64_t)(c->w * c->tw / 2.f);
        t.tile_h = (uint32_t)(uint64_t)(c->h * c->th / 2.f);
    } else {
        t.tiles_w = t.tiles_h = 1;
        t.tile_w = c->w; t.tile_h = c->h;
    }
    t.stride = t.tile_w * t.tiles_w;
    return t;
}

// A frame can be made (rays set); the context's device is made current.
int check_ready(vrt_hip_ctx *c)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!c->rays_set || !c->w || !c->h) return fail(c, VRT_HIP_ERR_INVALID, "render: call vrt_hip_set_plane/set_camera first");
    HIPCHK(c, hipSetDevice(c->device));
    return VRT_HIP_OK;
}

// (Re)builds the tile-centre arrays when the tile grid changes (the reference's float loops, rt.cpp:47-49).
int prepare_tile_grid(vrt_hip_ctx *c, float tw, float th)
{
    { int rc = quiesce(c); if (rc) return rc; } // xc / yc / w_start are read by list kernels in flight
    std::vector<float> xc, yc;
    for (float x = -1.f + tw / 2; x < 1.f; x += tw) { xc.push_back(x); if (xc.size() > 4096) break; }
    for (float y = -1.f + th / 2; y < 1.f; y += th) { yc.push_back(y); if (yc.size() > 4096) break; }
    const uint32_t tiles_w = (uint32_t)std::ceil(2.f / tw), tiles_h = (uint32_t)std::ceil(2.f / th); // types.h:280
    if (xc.size() > 4096 || yc.size() > 4096 || tiles_w > 4096 || tiles_h > 4096)
        return fail(c, VRT_HIP_ERR_INVALID, "tile_gaussians: more than 4096 tiles per axis");
    // The reference indexes tiles.gaussians[ty*tiles.w + tx] for ty < tiles.h, tx < tiles.w (rt.h:356) while the
    // float loops produced xc.size() tiles per row; they agree unless 2/t is not representable.  Keep tiles.w x
    // tiles.h tiles, each tested against the centre the loops would have produced for that row/column.
    while (xc.size() < tiles_w) xc.push_back(xc.empty() ? -1.f + tw / 2 : xc.back() + tw);
    while (yc.size() < tiles_h) yc.push_back(yc.empty() ? -1.f + th / 2 : yc.back() + th);
    const size_t nt = (size_t)tiles_w * tiles_h;
    if (nt * (size_t)std::max(c->n, 1u) > (size_t)1 << 31)
        return fail(c, VRT_HIP_ERR_NOMEM, "tile_gaussians: tiles x gaussians too large");
    HIPCHK(c, c->xc.reserve(tiles_w)); HIPCHK(c, c->yc.reserve(tiles_h));
    HIPCHK(c, c->w_start.reserve(nt)); HIPCHK(c, c->w_count.reserve(nt)); HIPCHK(c, c->w_indices.reserve(nt * c->n));
    std::vector<uint32_t> start(nt);
    for (size_t t = 0; t < nt; ++t) start[t] = (uint32_t)(t * c->n);
    HIPCHK(c, hipMemcpy(c->xc.p, xc.data(), tiles_w * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->yc.p, yc.data(), tiles_h * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->w_start.p, start.data(), nt * 4, hipMemcpyHostToDevice));
    c->grid_tw = tw; c->grid_th = th; c->grid_n = c->n;
    if (c->tile_mode != TILES_DEVICE || c->tiles_w != tiles_w || c->tiles_h != tiles_h) c->shard_dirty = true;
    // another tile grid = other cell lists, other cells beyond dense_threshold: launch reports of the old grid say nothing
    // about this one (round-2 advisor finding: the dense launch was left out on the first frame of a new grid)
    c->reset_seq = c->frame_seq;
    c->tile_mode = TILES_DEVICE; c->tw = tw; c->th = th; c->tiles_w = tiles_w; c->tiles_h = tiles_h;
    return VRT_HIP_OK;
}

// The single-tile "everything" list of the untiled overloads (rt.h:227-228, 315-316).
int ensure_none_ref_lists(vrt_hip_ctx *c)
{
    if (c->tile_mode != TILES_NONE || c->ref_valid) return VRT_HIP_OK;
    HIPCHK(c, c->ref_start.reserve(1)); HIPCHK(c, c->ref_count.reserve(1));
    const uint32_t zero = 0, n = c->n;
    HIPCHK(c, hipMemcpy(c->ref_start.p, &zero, 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ref_count.p, &n, 4, hipMemcpyHostToDevice));
    c->ref_valid = true;
    return VRT_HIP_OK;
}

namespace {

// Reference-semantics lists of the device binning (what tiles_t would hold), on the context's stream: built by
// vrt_hip_tile_gaussians, or on demand for queries (get_tile_counts / get_tile_indices).
int launch_device_ref_lists(vrt_hip_ctx *c)
{
    const size_t nt = (size_t)c->tiles_w * c->tiles_h;
    HIPCHK(c, c->ref_count.reserve(nt)); HIPCHK(c, c->ref_indices.reserve(nt * c->n));
    BinArgs a = bin_args(c);
    a.refine = 0;
    a.out_start = c->w_start.p; a.out_indices = c->ref_indices.p; a.out_count = c->ref_count.p;
    launch_build_tile_lists(a, FuseArgs{}, false, (uint32_t)nt, c->stream);
    HIPCHK(c, hipGetLastError());
    return VRT_HIP_OK;
}

// The reference-semantics lists ready to be read on the host.
int sync_ref_lists(vrt_hip_ctx *c)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (c->tile_mode == TILES_DEVICE && !c->ref_valid) {
        int rc = launch_device_ref_lists(c);
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ref_valid = true;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VRT_HIP_OK;
}

// Owner of tile t = (tx, ty): the ranks form an a x b brick (a * b = world, a >= b as square as the divisors allow) that
// tiles the tile grid, every row of bricks shifted by half a brick against the one above:
// owner = (tx + (a / 2) * (ty / b)) % a + a * (ty % b).  Every a x b window of tiles, wherever it lies, holds every rank once,
// so an object that covers a few tiles in the middle of the frame -- `-g 64 -w 2048` lights 4 x 4 of the 16 x 16 tiles, the
// outer ones partly -- is spread evenly: the busiest of 8 ranks gets 12.8 % of its cells (ideal 12.5 %; unshifted bricks
// 14.3 %, because a rank's two tiles then share a column; dealing tiles along diagonals, as round 1 did, 25 %).
// sharding.py mirrors this.
inline int shard_owner(uint32_t t, uint32_t tiles_w, int world)
{
    uint32_t b = 1;
    for (uint32_t d = 1; d * d <= (uint32_t)world; ++d)
        if ((uint32_t)world % d == 0) b = d;
    const uint32_t a = (uint32_t)world / b;
    const uint32_t tx = t % tiles_w, ty = t / tiles_w;
    return (int)((tx + (a / 2) * (ty / b)) % a + a * (ty % b));
}

} // namespace

int rebuild_shard(vrt_hip_ctx *c)
{
    if (!c->shard_dirty) return VRT_HIP_OK;
    const bool tiled = c->tile_mode != TILES_NONE;
    const uint32_t tiles_w = tiled ? c->tiles_w : 1, ntiles = tiled ? c->tiles_w * c->tiles_h : 1;
    std::vector<std::vector<uint32_t>> owned(c->world);
    for (uint32_t t = 0; t < ntiles; ++t) owned[shard_owner(t, tiles_w, c->world)].push_back(t);
    size_t slots = 0;
    for (auto &v : owned) slots = std::max(slots, v.size());
    std::vector<uint32_t> slot_tiles((size_t)c->world * slots, 0xFFFFFFFFu);
    for (int r = 0; r < c->world; ++r)
        for (size_t k = 0; k < owned[r].size(); ++k) slot_tiles[(size_t)r * slots + k] = owned[r][k];
    c->n_local = (uint32_t)owned[c->rank].size();
    c->n_slots = (uint32_t)slots;
    HIPCHK(c, c->tile_map.reserve(c->n_local)); HIPCHK(c, c->slot_tiles.reserve(slot_tiles.size()));
    if (c->n_local)
        HIPCHK(c, hipMemcpy(c->tile_map.p, owned[c->rank].data(), c->n_local * 4, hipMemcpyHostToDevice));
    if (!slot_tiles.empty())
        HIPCHK(c, hipMemcpy(c->slot_tiles.p, slot_tiles.data(), slot_tiles.size() * 4, hipMemcpyHostToDevice));
    c->shard_dirty = false;
    return VRT_HIP_OK;
}

uint32_t sparse_capacity(vrt_hip_ctx *c)
{
    if (rebuild_shard(c)) return 0;
    const TileLists t = tile_geometry(c);
    const uint32_t cx = (t.tile_w + CELL - 1) / CELL, cy = (t.tile_h + CELL - 1) / CELL;
    return c->n_slots * cx * cy;
}

namespace {

// Are the plane arrays an affine function of (row, column)?  Then rays are a pinhole bundle and the
// corner rays of a tile bound its cone.  Anything else disables the tile-level cull (the per-block cull
// works from the actual lane rays and stays exact for arbitrary arrays).
bool plane_is_affine(uint32_t w, uint32_t h, const float *xs, const float *ys, const float *zs)
{
    const float *a[3] = { xs, ys, zs };
    for (int k = 0; k < 3; ++k) {
        const float *p = a[k];
        const double p00 = p[0];
        const double dx = w > 1 ? ((double)p[w - 1] - p00) / (w - 1) : 0.0;
        const double dy = h > 1 ? ((double)p[(size_t)(h - 1) * w] - p00) / (h - 1) : 0.0;
        double scale = 1.0;
        for (uint32_t i = 0; i < h; i += (h > 64 ? h / 64 : 1)) scale = std::max(scale, std::fabs((double)p[(size_t)i * w]));
        const double tol = 1e-5 * scale;
        for (uint32_t i = 0; i < h; ++i)
            for (uint32_t j = 0; j < w; ++j)
                if (std::fabs((double)p[(size_t)i * w + j] - (p00 + dx * j + dy * i)) > tol) return false;
    }
    return true;
}

// Caller-made lists index the scene they were validated against (set_tiles checks every index < n): they do not survive another
// scene -- back to untiled until set_tiles / tile_gaussians is called again
void untile(vrt_hip_ctx *c) { c->tile_mode = TILES_NONE; c->tw = c->th = 2.f; c->tiles_w = c->tiles_h = 1; }

// The one place the host runtime reads the environment: every VRT_HIP_* setting (Tuning), at vrt_hip_create.  Values out
// of range keep the default.
Tuning read_tuning()
{
    Tuning t;
    if (const char *e = getenv("VRT_HIP_RENDER_WAVES")) { const int v = atoi(e); if (v >= 1 && v <= 16) t.render_waves_per_cu = v; }
    if (const char *e = getenv("VRT_HIP_RENDER_GRID")) t.render_grid_override = (uint32_t)std::max(0, atoi(e));
    if (const char *e = getenv("VRT_HIP_CULL_REF_N")) t.cull_ref_n = fmaxf(0.f, (float)atof(e));
    if (const char *e = getenv("VRT_HIP_CHUNKS")) t.use_chunks = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("VRT_HIP_CULL_PRUNE")) t.cull_prune = fmaxf(0.f, (float)atof(e));
    if (const char *e = getenv("VRT_HIP_TABLE_STEP")) { const float v = (float)atof(e); if (v >= 0.f && v <= 1.f) t.table_step = v; }
    if (const char *e = getenv("VRT_HIP_TABLE_ROOM")) { const float v = (float)atof(e); if (v > 0.f && v <= 10.f) t.table_room = v; }
    if (const char *e = getenv("VRT_HIP_TABLE_ADAPT")) { const float v = (float)atof(e); if (v >= 1.f && v <= 3.f) t.table_adapt = v; }
    if (const char *e = getenv("VRT_HIP_TABLE_BUDGET")) { const float v = (float)atof(e); if (v > 0.f) t.table_budget = v; }
    if (const char *e = getenv("VRT_HIP_CLAIM_EARLY")) t.claim_early = std::max(0, atoi(e));
    if (const char *e = getenv("VRT_HIP_DENSE_SKIP")) t.skip_idle_dense = atoi(e) != 0;
    if (const char *e = getenv("VRT_HIP_DENSE_WAVES")) { const int v = atoi(e); if (v == 4 || v == 8 || v == 16 || v == 17) t.dense_waves = v; }
    if (const char *e = getenv("VRT_HIP_TIMELINE")) { t.timeline = true; if (strstr(e, ".csv")) t.timeline_csv = e; }
    t.table_diag = getenv("VRT_HIP_TABLE_DIAG") != nullptr;
    if (const char *e = getenv("VRT_HIP_RETAIN_FRAME")) t.retain_frame = atoi(e) != 0;
    if (const char *e = getenv("VRT_HIP_RAY_INDEX")) t.ray_index = atoi(e) != 0;
    if (const char *e = getenv("VRT_HIP_GRAD_ORDERED")) t.grad_ordered = atoi(e) != 0;
    if (const char *e = getenv("VRT_HIP_RAY_SORT")) t.ray_sort = atoi(e) != 0;
    return t;
}

} // namespace

extern "C" {

const char *vrt_hip_version(void) { return "vrt_hip 0.2 (gfx950)"; }

int vrt_hip_create(int device, vrt_hip_ctx **out)
{
    if (!out) return fail(nullptr, VRT_HIP_ERR_INVALID, "create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(nullptr, VRT_HIP_ERR_NO_DEVICE, "create: no HIP device visible (libvrt_hip has no CPU fallback)");
    if (device < 0 || device >= count) return fail(nullptr, VRT_HIP_ERR_INVALID, "create: device index out of range");
    HIPCHK(nullptr, hipSetDevice(device));
    vrt_hip_ctx *c = new (std::nothrow) vrt_hip_ctx();
    if (!c) return fail(nullptr, VRT_HIP_ERR_NOMEM, "create: out of host memory");
    c->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->num_cus = cus;
    PinnedBuf<volatile uint32_t> fb;
    void *dp = nullptr;
    if (fb.alloc(4, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dp, (void *)fb.p, 0) == hipSuccess) {
        memset((void *)fb.p, 0, 4 * sizeof(uint32_t));
        c->h_fb = std::move(fb); c->d_fb = (uint32_t *)dp;
    }
    c->tune = read_tuning();
    c->cull_prune = c->tune.cull_prune; c->table_hx = c->tune.table_step; c->table_budget = c->tune.table_budget;
    c->ray_index = c->tune.ray_index;
    c->grad_ordered = c->tune.grad_ordered;
    c->ray_sort = c->tune.ray_sort;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&c->scene_order, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->scene_done, hipEventDisableTiming) != hipSuccess ||
        c->d_stats.reserve(STAT_WORDS) != hipSuccess) {
        vrt_hip_destroy(c);
        return fail(nullptr, VRT_HIP_ERR_HIP, "create: stream/event creation failed");
    }
    *out = c;
    return VRT_HIP_OK;
}

void vrt_hip_destroy(vrt_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)quiesce(c); // frames still in flight on the context's stream or on the caller's last stream read its buffers
    c->host_regs.clear(); // the caller's host buffers: unregistered once nothing in flight can write them
    for (vrt_hip_ray_plan *p : c->plans) delete p; // the ray plans that were not destroyed
    c->plans.clear(); c->plan = nullptr;
    for (auto &e : c->batch_copied) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->tev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->scene_order) (void)hipEventDestroy(c->scene_order);
    if (c->scene_done) (void)hipEventDestroy(c->scene_done);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c; // the buffers free themselves
}

const char *vrt_hip_last_error(const vrt_hip_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int vrt_hip_set_gaussians(vrt_hip_ctx *c, size_t n, const float *mu_x, const float *mu_y, const float *mu_z,
                          const float *ar, const float *ag, const float *ab, const float *aa, const float *sigma,
                          const float *mag)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (n > 0xFFFFFFF0ull) return fail(c, VRT_HIP_ERR_INVALID, "set_gaussians: too many Gaussians");
    const float *src[9] = { mu_x, mu_y, mu_z, ar, ag, ab, aa, sigma, mag };
    for (int i = 0; i < 9; ++i)
        if (n && !src[i] && i != 6) return fail(c, VRT_HIP_ERR_INVALID, "set_gaussians: NULL array");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; }
    for (int i = 0; i < 9; ++i) {
        HIPCHK(c, c->soa[i].reserve(n));
        if (n && src[i]) HIPCHK(c, hipMemcpy(c->soa[i].p, src[i], n * sizeof(float), hipMemcpyHostToDevice));
    }
    c->has_alpha = aa != nullptr;
    // the cull bounds count a dropped Gaussian's emission at albedo <= 1 (the reference's range): brighter scenes shrink the prune's budget
    c->albedo_scale = 1.f;
    c->albedo_pending = false; c->scene_on_device = false;
    for (int ch = 3; ch <= 6; ++ch)
        if (src[ch])
            for (size_t i = 0; i < n; ++i) { const float v = fabsf(src[ch][i]); if (v > c->albedo_scale && v < INFINITY) c->albedo_scale = v; }
    c->n = (uint32_t)n;
    ++c->state_gen;
    ++c->cull_gen; c->cull_gen_why = "the Gaussians were set again (vrt_hip_set_gaussians)"; // a strict ray plan is stale
    c->reset_seq = c->frame_seq;
    c->tables_dirty = true;
    c->lists_dirty = true;
    if (c->tile_mode == TILES_HOST) { untile(c); c->shard_dirty = true; }
    c->ref_valid = false;
    return VRT_HIP_OK;
}

int vrt_hip_set_gaussians_aos(vrt_hip_ctx *c, size_t n, const void *gaussians)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (n && !gaussians) return fail(c, VRT_HIP_ERR_INVALID, "set_gaussians_aos: NULL");
    // gaussian_t: albedo[4] mu[4] sigma magnitude (types.h:195-200)
    const float *g = (const float *)gaussians;
    std::vector<float> soa[9];
    for (auto &v : soa) v.resize(n ? n : 1);
    for (size_t i = 0; i < n; ++i) {
        const float *p = g + 10 * i;
        soa[3][i] = p[0]; soa[4][i] = p[1]; soa[5][i] = p[2]; soa[6][i] = p[3];
        soa[0][i] = p[4]; soa[1][i] = p[5]; soa[2][i] = p[6];
        soa[7][i] = p[8]; soa[8][i] = p[9];
    }
    return vrt_hip_set_gaussians(c, n, soa[0].data(), soa[1].data(), soa[2].data(), soa[3].data(), soa[4].data(),
                                 soa[5].data(), soa[6].data(), soa[7].data(), soa[8].data());
}

// The scene from device memory: what vrt_hip_set_gaussians and the table build of rebuild_tables do, as kernels on the caller's stream
// and with no wait (include/vrt_hip.h has the contract).  Work of the context's own stream is ordered by two events, never by the host.
int vrt_hip_set_gaussians_device(vrt_hip_ctx *c, size_t n, const float *d_mu, const float *d_albedo, const float *d_sigma,
                                 const float *d_magnitude, void *hip_stream)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (n > 0xFFFFFFF0ull) return fail(c, VRT_HIP_ERR_INVALID, "set_gaussians_device: too many Gaussians");
    if (n && (!d_mu || !d_albedo || !d_sigma || !d_magnitude)) return fail(c, VRT_HIP_ERR_INVALID, "set_gaussians_device: NULL array");
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(c, hipSetDevice(c->device));
    wait_for_last_stream(c, st); // frames and bundles in flight on another stream read what this rewrites
    c->last_stream = st;
    HIPCHK(c, hipEventRecord(c->scene_order, c->stream)); // ... and so may work on the context's own stream
    HIPCHK(c, hipStreamWaitEvent(st, c->scene_order, 0));
    // (a buffer that grows is freed first, which waits for the device: nothing in flight loses its memory)
    SceneColumns cols;
    for (int i = 0; i < 9; ++i) { HIPCHK(c, c->soa[i].reserve(n)); cols.c[i] = c->soa[i].p; }
    HIPCHK(c, c->mu_sig.reserve(n)); HIPCHK(c, c->gA.reserve(n)); HIPCHK(c, c->gB.reserve(n));
    HIPCHK(c, c->gC.reserve(n)); HIPCHK(c, c->gD.reserve(n)); HIPCHK(c, c->iota.reserve(n));
    HIPCHK(c, c->gChunk.reserve((n + 63u) / 64u));
    HIPCHK(c, c->scene_words.reserve(8));
    HIPCHK(c, hipMemsetAsync(c->scene_words.p + 6, 0, sizeof(uint32_t), st));
    const uint32_t un = (uint32_t)n;
    launch_ingest_scene(un, d_mu, d_albedo, d_sigma, d_magnitude, cols, c->scene_words.p + 6, st);
    const float eps_eff = c->cull_eps * std::min(1.f, 4096.f / (float)std::max(un, 1u)); // as rebuild_tables
    launch_build_static(un, c->soa[0].p, c->soa[1].p, c->soa[2].p, c->soa[3].p, c->soa[4].p, c->soa[5].p, c->soa[6].p, c->soa[7].p,
                        c->soa[8].p, eps_eff, exp_floor_x(c->exp_kind), c->mu_sig.p, c->gB.p, c->gC.p, c->gD.p, st);
    launch_build_chunks(un, c->mu_sig.p, c->gB.p, c->gChunk.p, st);
    launch_iota(c->iota.p, un, st);
    HIPCHK(c, hipGetLastError());
    c->has_alpha = true;
    c->n = un;
    c->scene_on_device = true;
    ++c->state_gen;
    ++c->cull_gen; c->cull_gen_why = "the Gaussians were set again (vrt_hip_set_gaussians_device)"; // a strict ray plan is stale
    c->reset_seq = c->frame_seq;
    c->tables_dirty = false; // built eagerly; a later change of cull_eps or the Exp kind rebuilds them from soa, as after any setter
    c->ray_index_dirty = true;
    c->gA_valid = false;
    c->lists_dirty = true;
    if (c->tile_mode == TILES_HOST) { untile(c); c->shard_dirty = true; }
    c->ref_valid = false;
    if (c->ray_index) { int rc = build_ray_index_device(c, st); if (rc) return rc; }
    c->albedo_pending = true; // the word is read by the first call that needs albedo_scale (resolve_albedo_scale)
    HIPCHK(c, hipEventRecord(c->scene_done, st));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->scene_done, 0)); // queries and frames on the context's stream see this scene
    return VRT_HIP_OK;
}

uint64_t vrt_hip_state_generation(const vrt_hip_ctx *c) { return c ? c->state_gen : 0; }

int vrt_hip_get_image_size(const vrt_hip_ctx *c, uint32_t *w, uint32_t *h)
{
    if (!c || !c->rays_set) return VRT_HIP_ERR_INVALID;
    if (w) *w = c->w;
    if (h) *h = c->h;
    return VRT_HIP_OK;
}

int vrt_hip_copy_state(vrt_hip_ctx *dst, const vrt_hip_ctx *src)
{
    if (!dst || !src || dst == src) return VRT_HIP_ERR_INVALID;
    if (dst->device != src->device) return fail(dst, VRT_HIP_ERR_INVALID, "copy_state: the contexts live on different devices");
    HIPCHK(dst, hipSetDevice(dst->device));
    { int rc = quiesce(dst); if (rc) return rc; }
    HIPCHK(dst, hipStreamSynchronize(src->stream)); // uploads of the source are synchronous, its table build runs on its stream
    // a source set from device memory: its columns are there once its update is done, and so is the word albedo_scale is read from
    if (resolve_albedo_scale(const_cast<vrt_hip_ctx *>(src))) return fail(dst, VRT_HIP_ERR_HIP, "copy_state: " + src->err);
    for (int i = 0; i < 9; ++i) {
        HIPCHK(dst, dst->soa[i].reserve(src->n));
        if (src->n && src->soa[i].p) HIPCHK(dst, hipMemcpy(dst->soa[i].p, src->soa[i].p, (size_t)src->n * sizeof(float), hipMemcpyDeviceToDevice));
    }
    dst->has_alpha = src->has_alpha; dst->n = src->n; dst->albedo_scale = src->albedo_scale;
    dst->albedo_pending = false; dst->scene_on_device = false;
    dst->exp_kind = src->exp_kind; dst->erf_kind = src->erf_kind; dst->cull_eps = src->cull_eps; dst->cull_prune = src->cull_prune;
    dst->table_hx = src->table_hx; dst->table_budget = src->table_budget; dst->tune.table_adapt = src->tune.table_adapt; dst->tune.table_room = src->tune.table_room;
    dst->rank = src->rank; dst->world = src->world;
    dst->grad_ordered = src->grad_ordered;
    dst->ray_sort = src->ray_sort;
    dst->ray_index = src->ray_index; // the mirror builds the same index with its tables: the order is a function of the scene alone
    dst->tables_dirty = true; dst->lists_dirty = true; dst->shard_dirty = true; dst->ref_valid = false;
    dst->reset_seq = dst->frame_seq;
    if (dst->tile_mode == TILES_HOST) untile(dst);
    ++dst->state_gen;
    ++dst->cull_gen; dst->cull_gen_why = "the scene was copied in (vrt_hip_copy_state)"; // another scene: the plans and the binding of dst stay its own, and a strict one is stale
    return VRT_HIP_OK;
}

int vrt_hip_set_options(vrt_hip_ctx *c, int exp_kind, int erf_kind, float cull_eps)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (exp_kind < 0 || exp_kind > VRT_EXP_SPLINE || erf_kind < 0 || erf_kind > VRT_ERF_TAYLOR || !(cull_eps >= 0.f))
        return fail(c, VRT_HIP_ERR_INVALID, "set_options: bad argument");
    const bool supported = (erf_kind == VRT_ERF_AS) || (exp_kind == VRT_EXP_VCL) ||
                           (exp_kind == VRT_EXP_LIBM && erf_kind == VRT_ERF_LIBM);
    if (!supported) return fail(c, VRT_HIP_ERR_INVALID, "set_options: this Exp/Erf pair is not instantiated");
    if (exp_kind != c->exp_kind || cull_eps != c->cull_eps) c->tables_dirty = true;
    if (exp_kind != c->exp_kind || erf_kind != c->erf_kind || cull_eps != c->cull_eps) { c->reset_seq = c->frame_seq; ++c->cull_gen; c->cull_gen_why = "cull_eps or the Exp / Erf pair changed (vrt_hip_set_options)"; /* a strict ray plan is stale */ }
    c->exp_kind = exp_kind; c->erf_kind = erf_kind; c->cull_eps = cull_eps;
    ++c->state_gen;
    return VRT_HIP_OK;
}

int vrt_hip_set_table_step(vrt_hip_ctx *c, float hx)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!(hx >= 0.f) || hx > 1.f) return fail(c, VRT_HIP_ERR_INVALID, "set_table_step: step must be in [0, 1]");
    if (hx != c->table_hx) { c->reset_seq = c->frame_seq; c->lists_dirty = true; }
    c->table_hx = hx;
    ++c->state_gen;
    return VRT_HIP_OK;
}

int vrt_hip_set_table_budget(vrt_hip_ctx *c, float budget)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!(budget > 0.f)) return fail(c, VRT_HIP_ERR_INVALID, "set_table_budget: the budget must be positive (INFINITY = unchecked)");
    if (budget != c->table_budget) c->reset_seq = c->frame_seq;
    c->table_budget = budget;
    ++c->state_gen;
    return VRT_HIP_OK;
}

int vrt_hip_set_cull_prune(vrt_hip_ctx *c, float kappa)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!(kappa >= 0.f)) return fail(c, VRT_HIP_ERR_INVALID, "set_cull_prune: the factor must be >= 0 (0 = off)");
    if (kappa != c->cull_prune) c->reset_seq = c->frame_seq;
    c->cull_prune = kappa;
    ++c->state_gen;
    return VRT_HIP_OK;
}

int vrt_hip_set_grad_ordered(vrt_hip_ctx *c, int on)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // bundles in flight keep the path they were enqueued with
    c->grad_ordered = on != 0;
    ++c->state_gen;
    return VRT_HIP_OK;
}

int vrt_hip_set_ray_sort(vrt_hip_ctx *c, int on)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // bundles in flight keep the order they were enqueued with
    c->ray_sort = on != 0;
    ++c->state_gen;
    return VRT_HIP_OK;
}

int vrt_hip_set_ray_index(vrt_hip_ctx *c, int on)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // bundles in flight keep the cull they were enqueued with
    c->ray_index = on != 0; // the index itself is made with the tables, or by the next bundle if they are already there
    ++c->state_gen;
    return VRT_HIP_OK;
}

int vrt_hip_clear_tiles(vrt_hip_ctx *c)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (c->tile_mode != TILES_NONE) c->reset_seq = c->frame_seq;
    untile(c);
    c->shard_dirty = true; c->lists_dirty = true; c->ref_valid = false;
    return VRT_HIP_OK;
}

int vrt_hip_set_tiles(vrt_hip_ctx *c, float tw, float th, uint64_t tiles_w, uint64_t tiles_h, const uint32_t *offsets,
                      const uint32_t *indices)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!offsets || tiles_w == 0 || tiles_h == 0 || tiles_w * tiles_h > (1u << 24) || !(tw > 0.f) || !(th > 0.f))
        return fail(c, VRT_HIP_ERR_INVALID, "set_tiles: bad argument");
    const size_t nt = (size_t)(tiles_w * tiles_h);
    const size_t total = offsets[nt];
    if (total && !indices) return fail(c, VRT_HIP_ERR_INVALID, "set_tiles: NULL indices");
    std::vector<uint32_t> start(nt), count(nt);
    for (size_t t = 0; t < nt; ++t) {
        if (offsets[t + 1] < offsets[t]) return fail(c, VRT_HIP_ERR_INVALID, "set_tiles: offsets not monotone");
        start[t] = offsets[t]; count[t] = offsets[t + 1] - offsets[t];
    }
    for (size_t k = 0; k < total; ++k)
        if (indices[k] >= c->n) return fail(c, VRT_HIP_ERR_INVALID, "set_tiles: index out of range (upload the scene first)");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; }
    c->ref_indices = {}; // exact-size index buffer: plan_lists (vrt_hip_frame.cpp) sizes its output from ref_indices.cap
    HIPCHK(c, c->ref_start.reserve(nt)); HIPCHK(c, c->ref_count.reserve(nt)); HIPCHK(c, c->ref_indices.reserve(total));
    HIPCHK(c, hipMemcpy(c->ref_start.p, start.data(), nt * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ref_count.p, count.data(), nt * 4, hipMemcpyHostToDevice));
    if (total) HIPCHK(c, hipMemcpy(c->ref_indices.p, indices, total * 4, hipMemcpyHostToDevice));
    c->reset_seq = c->frame_seq;
    c->tile_mode = TILES_HOST; c->tw = tw; c->th = th; c->tiles_w = (uint32_t)tiles_w; c->tiles_h = (uint32_t)tiles_h;
    c->shard_dirty = true; c->lists_dirty = true; c->ref_valid = true;
    return VRT_HIP_OK;
}

int vrt_hip_tile_gaussians_device(vrt_hip_ctx *c, float tw, float th, const float view[16], void *hip_stream)
{
    (void)hip_stream; // the lists are built by the next render on ITS stream (they depend on its rays and origin)
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!view || !(tw > 0.f) || !(th > 0.f)) return fail(c, VRT_HIP_ERR_INVALID, "tile_gaussians: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = rebuild_tables(c);
    if (rc) return rc;
    if (c->tile_mode != TILES_DEVICE || c->grid_tw != tw || c->grid_th != th || c->grid_n != c->n) {
        if ((rc = prepare_tile_grid(c, tw, th))) return rc; // waits for frames in flight (quiesce)
    }
    if (memcmp(c->view, view, 16 * sizeof(float))) c->cam_seq = c->frame_seq;
    memcpy(c->view, view, 16 * sizeof(float));
    c->lists_dirty = true;
    c->ref_valid = false;
    return VRT_HIP_OK;
}

int vrt_hip_tile_gaussians(vrt_hip_ctx *c, float tw, float th, const float view[16])
{
    if (!c) return VRT_HIP_ERR_INVALID;
    int rc = vrt_hip_tile_gaussians_device(c, tw, th, view, nullptr);
    if (rc) return rc;
    // the synchronous form also materialises the reference-semantics lists (what tiles_t would hold), timed
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if ((rc = launch_device_ref_lists(c))) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last.tiling_ms = ms;
    c->ref_valid = true;
    return VRT_HIP_OK;
}

int vrt_hip_get_tile_counts(vrt_hip_ctx *c, uint32_t *counts, size_t cap, uint64_t *tiles_w, uint64_t *tiles_h)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (c->tile_mode == TILES_NONE) return fail(c, VRT_HIP_ERR_INVALID, "get_tile_counts: no tiles set");
    const size_t nt = (size_t)c->tiles_w * c->tiles_h;
    if (tiles_w) *tiles_w = c->tiles_w;
    if (tiles_h) *tiles_h = c->tiles_h;
    if (counts) {
        if (cap < nt) return fail(c, VRT_HIP_ERR_INVALID, "get_tile_counts: buffer too small");
        int rc = sync_ref_lists(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(counts, c->ref_count.p, nt * 4, hipMemcpyDeviceToHost));
    }
    return VRT_HIP_OK;
}

int vrt_hip_get_tile_indices(vrt_hip_ctx *c, uint64_t t, uint32_t *indices, size_t cap, uint32_t *count)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (c->tile_mode == TILES_NONE || t >= (uint64_t)c->tiles_w * c->tiles_h)
        return fail(c, VRT_HIP_ERR_INVALID, "get_tile_indices: bad tile");
    int rc = sync_ref_lists(c);
    if (rc) return rc;
    const uint32_t *starts = c->tile_mode == TILES_DEVICE ? c->w_start.p : c->ref_start.p;
    uint32_t start = 0, cnt = 0;
    HIPCHK(c, hipMemcpy(&start, starts + t, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&cnt, c->ref_count.p + t, 4, hipMemcpyDeviceToHost));
    if (count) *count = cnt;
    if (indices) {
        if (cap < cnt) return fail(c, VRT_HIP_ERR_INVALID, "get_tile_indices: buffer too small");
        if (cnt) HIPCHK(c, hipMemcpy(indices, c->ref_indices.p + start, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    }
    return VRT_HIP_OK;
}

int vrt_hip_set_plane(vrt_hip_ctx *c, uint32_t w, uint32_t h, const float *xs, const float *ys, const float *zs)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!w || !h || !xs || !ys || !zs) return fail(c, VRT_HIP_ERR_INVALID, "set_plane: bad argument");
    const size_t n = (size_t)w * h;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; }
    HIPCHK(c, c->xs.reserve(n)); HIPCHK(c, c->ys.reserve(n)); HIPCHK(c, c->zs.reserve(n));
    HIPCHK(c, hipMemcpy(c->xs.p, xs, n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ys.p, ys, n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->zs.p, zs, n * 4, hipMemcpyHostToDevice));
    c->plane_affine = plane_is_affine(w, h, xs, ys, zs);
    c->reset_seq = c->frame_seq; // new rays
    c->w = w; c->h = h; c->plane_mode = true; c->rays_set = true; c->lists_dirty = true;
    ++c->plane_gen; // other plane arrays behind the same pointers: the tile cones are no longer theirs
    return VRT_HIP_OK;
}

int vrt_hip_set_camera(vrt_hip_ctx *c, uint32_t w, uint32_t h, const float pos[3], const float right[3],
                       const float up[3], const float front[3], float focal)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!w || !h || !pos || !right || !up || !front) return fail(c, VRT_HIP_ERR_INVALID, "set_camera: bad argument");
    if (c->w != w || c->h != h || c->plane_mode || c->focal != focal || memcmp(c->cam_pos, pos, 12) || memcmp(c->cam_right, right, 12) ||
        memcmp(c->cam_up, up, 12) || memcmp(c->cam_front, front, 12))
        (c->w != w || c->h != h ? c->reset_seq : c->cam_seq) = c->frame_seq; // another camera / another image size
    memcpy(c->cam_pos, pos, 12); memcpy(c->cam_right, right, 12); memcpy(c->cam_up, up, 12); memcpy(c->cam_front, front, 12);
    c->focal = focal; c->w = w; c->h = h; c->plane_mode = false; c->view_mode = false; c->rays_set = true; c->lists_dirty = true;
    return VRT_HIP_OK;
}

int vrt_hip_set_camera_view(vrt_hip_ctx *c, uint32_t w, uint32_t h, const float view[16])
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!w || !h || !view) return fail(c, VRT_HIP_ERR_INVALID, "set_camera_view: bad argument");
    float inv[16];
    vrt_hip_mat4_inverse(view, inv); // glm::inverse in glm's order, unfused (csrc/vrt_host_camera.cpp)
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(inv[i])) return fail(c, VRT_HIP_ERR_INVALID, "set_camera_view: the view matrix is singular");
    if (c->w != w || c->h != h || c->plane_mode || !c->view_mode || memcmp(c->inv_view, inv, sizeof inv))
        (c->w != w || c->h != h ? c->reset_seq : c->cam_seq) = c->frame_seq; // another camera / another image size
    memcpy(c->inv_view, inv, sizeof inv);
    c->w = w; c->h = h; c->plane_mode = false; c->view_mode = true; c->rays_set = true; c->lists_dirty = true;
    return VRT_HIP_OK;
}

size_t vrt_hip_image_pixels(const vrt_hip_ctx *c) { return (c && c->rays_set) ? (size_t)c->w * c->h : 0; }

int vrt_hip_sync(vrt_hip_ctx *c)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VRT_HIP_OK;
}

int vrt_hip_set_shard(vrt_hip_ctx *c, int rank, int world)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, VRT_HIP_ERR_INVALID, "set_shard: bad rank/world");
    if (rank != c->rank || world != c->world) ++c->state_gen; // vrt_hip_copy_state copies rank / world: holders of mirrors must see the change
    c->rank = rank; c->world = world; c->shard_dirty = true; c->lists_dirty = true; c->reset_seq = c->frame_seq;
    return VRT_HIP_OK;
}

size_t vrt_hip_shard_pixels(const vrt_hip_ctx *cc)
{
    vrt_hip_ctx *c = const_cast<vrt_hip_ctx *>(cc);
    if (!c || !c->rays_set) return 0;
    if (rebuild_shard(c)) return 0;
    const TileLists t = tile_geometry(c);
    return (size_t)c->n_slots * t.tile_w * t.tile_h;
}

// ---- sparse shards: only the cells some Gaussian reaches travel (multi-GPU transport) ------------------------------
size_t vrt_hip_sparse_shard_words(const vrt_hip_ctx *cc)
{
    vrt_hip_ctx *c = const_cast<vrt_hip_ctx *>(cc);
    if (!c || !c->rays_set) return 0;
    const uint32_t cap = sparse_capacity(c);
    return sparse_pixel_offset(cap) + (size_t)cap * CELL * CELL;
}

} // extern "C"
