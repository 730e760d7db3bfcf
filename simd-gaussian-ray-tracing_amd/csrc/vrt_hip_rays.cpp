// vrt_hip_rays.cpp -- ray bundles of libvrt_hip.so (vrt_hip_radiance_rays*, vrt_hip_transmittance_bundle*, vrt_hip_depth_bundle*,
// vrt_hip_radiance_rays_grad*, vrt_hip_transmittance_bundle_grad*, their _rays forms, vrt_hip_radiance_rays_gn_diag*, vrt_hip_radiance_rays_tangent*, vrt_hip_transmittance_bundle_tangent*): radiance of caller-given rays, transmittance at sample distances along
// them, the distance at which their transmittance falls to given levels, or the derivative of their radiance, transmittance or depth with
// respect to the Gaussians, or how their radiance, transmittance or depth moves along a direction (forward mode), culled per ray (vrt_ray_kernel.hip,
// vrt_ray_trans_kernel.hip, vrt_ray_depth_kernel.hip, vrt_ray_grad_kernel.hip, vrt_ray_trans_grad_kernel.hip, vrt_ray_tangent_kernel.hip, vrt_ray_trans_tangent_kernel.hip).  The scene tables and the
// chunk spheres are the frame pipeline's; the long-ray queue, its counters and the long kernel's scratch slots belong to the context
// and only grow.  So do the buffers of the ordered gradient tables (vrt_hip_set_grad_ordered: ordered_bundle, and the two read-outs)
// and of the sorted bundles (vrt_hip_set_ray_sort: sort_bundle, and the two read-outs).  Ray plans (vrt_hip_ray_plan_create*,
// vrt_hip_set_ray_plan, at the end of this file) own their memory: a bundle enqueued while one is bound reads its lists, its queue and its
// order from it and reserves neither queue nor scratch slots.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <numeric>

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

// 10 bits spread to every third bit
uint32_t spread3(uint32_t v)
{
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

bool finite_centre(const float4 &p) { return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z); }

// perm[Morton position] = scene index (build_ray_index says how the key is made)
std::vector<uint32_t> morton_order(const std::vector<float4> &ms)
{
    const uint32_t n = (uint32_t)ms.size();
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (const float4 &p : ms) {
        if (!finite_centre(p)) continue;
        const float v[3] = { p.x, p.y, p.z };
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
    }
    std::vector<uint32_t> key(n), perm(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (!finite_centre(ms[i])) { key[i] = 0; continue; }
        const float v[3] = { ms[i].x, ms[i].y, ms[i].z };
        uint32_t k = 0;
        for (int a = 0; a < 3; ++a) {
            const double ext = (double)hi[a] - (double)lo[a];
            const uint32_t q = ext > 0.0 ? (uint32_t)std::min(1023.0, std::floor(((double)v[a] - (double)lo[a]) / ext * 1024.0)) : 0u;
            k |= spread3(q) << a;
        }
        key[i] = k;
    }
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    return perm;
}

// What a bundle of any kind (radiance, transmittance, depth, gradient) enqueues before its two kernels: the tables brought up to date, the Morton
// index when it is on and out of date, the queue / counters / scratch / statistics buffers at their size for nrays, the counters (and
// statistics) cleared on the stream, and the kernels' arguments but for the outputs, which the caller fills in.
struct Bundle {
    RayArgs a{};
    uint32_t grid = 0;
    int src = RAY_LIST_CHUNKS; // where the kernels take the lists from (RayListSource)
};
// A bundle while vrt_hip_set_ray_sort is on (include/vrt_hip.h has the contract, vrt_ray_sort_kernel.hip the two steps): the keys by the
// sphere tests of the cull the bundle will run, the stable sort, and a.order for the lane = ray kernels behind them -- all on the call's
// stream.  A bundle of one wave has nothing to regroup and is not sorted.  The storage query is the host's, from nrays; a buffer that
// grows is freed first, which waits for the device, and a call whose buffers are large enough waits for nothing.
int sort_bundle(vrt_hip_ctx *c, RayArgs &a, bool indexed, hipStream_t st)
{
    const size_t nrays = (size_t)a.nrays;
    c->rs_last_valid = true; c->rs_last_sorted = false; c->rs_last_rays = nrays;
    if (!c->ray_sort || nrays <= 64) return VRT_HIP_OK;
    const uint32_t spheres = (c->n + 63u) / 64u, bits = ray_sort_field_bits(spheres);
    if (c->rs_sort_n != nrays || c->rs_sort_bits != bits) {
        c->rs_sort_bytes = ray_sort_bytes(nrays, spheres);
        if (!c->rs_sort_bytes) return fail(c, VRT_HIP_ERR_HIP, "ray sort: the sort's storage query failed");
        c->rs_sort_n = nrays; c->rs_sort_bits = bits;
    }
    HIPCHK(c, c->rs_keys.reserve(nrays)); HIPCHK(c, c->rs_ids.reserve(nrays)); HIPCHK(c, c->rs_keys_sorted.reserve(nrays));
    HIPCHK(c, c->rs_order.reserve(nrays)); HIPCHK(c, c->rs_none.reserve(1)); HIPCHK(c, c->rs_sort_tmp.reserve(c->rs_sort_bytes));
    RaySort o{};
    o.keys = c->rs_keys.p; o.ids = c->rs_ids.p; o.keys_sorted = c->rs_keys_sorted.p; o.order = c->rs_order.p; o.none = c->rs_none.p;
    o.spheres = spheres; o.sort_tmp = c->rs_sort_tmp.p; o.sort_bytes = c->rs_sort_bytes;
    HIPCHK(c, launch_ray_sort(a, indexed, o, st));
    a.order = c->rs_order.p;
    c->rs_last_sorted = true; c->rs_last_spheres = spheres;
    return VRT_HIP_OK;
}

int enqueue_bundle(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs, hipStream_t st, Bundle &b)
{
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = rebuild_tables(c); if (rc) return rc; }
    // a bound ray plan (vrt_hip_set_ray_plan) gives every ray its list: no index, no sort, no queue and no scratch slot take part
    const vrt_hip_ray_plan *plan = c->plan;
    const int src = plan ? RAY_LIST_PLAN : c->ray_index ? RAY_LIST_INDEX : RAY_LIST_CHUNKS;
    const bool indexed = src == RAY_LIST_INDEX;
    if (indexed && c->ray_index_dirty) { // switched on after the tables were made
        { int rc = quiesce(c); if (rc) return rc; }
        if (c->scene_on_device) { // its tables were made on the device: so is its index, on the context's stream like the host's build
            { int rc = build_ray_index_device(c, c->stream); if (rc) return rc; }
            HIPCHK(c, hipStreamSynchronize(c->stream)); // bundles may use a caller's stream
        } else { int rc = build_ray_index(c); if (rc) return rc; }
    }
    wait_for_last_stream(c, st); // a bundle in flight on another stream uses the queue and the scratch slots
    c->last_stream = st;
    const uint32_t grid = long_grid(c);
    // (a buffer that grows is freed first, which waits for the device: no bundle in flight loses its memory)
    if (!plan) HIPCHK(c, c->ray_queue.reserve(nrays));
    HIPCHK(c, c->ray_counters.reserve(2));
    if (!plan) HIPCHK(c, c->ray_scratch.reserve((size_t)grid * c->n));
    constexpr size_t stats_words = RAY_STATS_WORDS + RAY_INDEX_STATS_WORDS;
    HIPCHK(c, c->ray_stats.reserve(stats_words));
    const uint32_t bitmap_words = (c->n + 31u) / 32u;
    if (indexed && c->ri_bitmap.cap < (size_t)grid * bitmap_words) { // new memory: all zero once, every ray leaves it so
        HIPCHK(c, c->ri_bitmap.reserve((size_t)grid * bitmap_words));
        HIPCHK(c, hipMemsetAsync(c->ri_bitmap.p, 0, c->ri_bitmap.cap * sizeof(uint32_t), st));
    }
    HIPCHK(c, hipMemsetAsync(c->ray_counters.p, 0, 2 * sizeof(uint32_t), st));
    if (c->stats_on) HIPCHK(c, hipMemsetAsync(c->ray_stats.p, 0, stats_words * sizeof(unsigned long long), st));
    c->ray_stats_valid = c->stats_on;
    c->ray_indexed_last = indexed; c->ri_last_leaves = (c->n + 63u) / 64u; c->ri_last_groups = (c->ri_last_leaves + 63u) / 64u;
    RayArgs &a = b.a;
    a.S = tables(c);
    a.chunks = c->gChunk.p;
    a.origins = d_origins; a.dirs = d_dirs; a.origin_per_ray = origin_per_ray ? 1 : 0;
    a.nrays = nrays;
    if (!plan) { a.queue = c->ray_queue.p; a.queue_cap = (uint32_t)nrays; a.scratch = c->ray_scratch.p; }
    a.counters = c->ray_counters.p; // [1], the long kernel's work counter, is the context's with a plan too
    a.stats = c->stats_on ? c->ray_stats.p : nullptr;
    if (indexed) {
        a.perm = c->ri_perm.p; a.mu_sig_m = c->ri_mu_sig.p; a.gB_m = c->ri_gB.p; a.leaves = c->ri_leaves.p; a.groups = c->ri_groups.p;
        a.bitmap = c->ri_bitmap.p;
        a.index_stats = c->stats_on ? c->ray_stats.p + RAY_STATS_WORDS : nullptr;
    }
    b.grid = grid; b.src = src;
    c->rs_last_plan = plan;
    if (plan) { // its lists, its queue and its order
        a.pl_len = plan->len.p; a.pl_off = plan->off.p; a.pl_entries = plan->list.p;
        a.pl_long = plan->long_ids.p; a.pl_nlong = (uint32_t)plan->long_rays;
        a.order = plan->sorted ? plan->order.p : nullptr;
        c->rs_last_valid = true; c->rs_last_sorted = plan->sorted; c->rs_last_rays = nrays; c->rs_last_spheres = plan->spheres;
        return VRT_HIP_OK;
    }
    return sort_bundle(c, a, indexed, st);
}

} // namespace

// The Morton index of the ray bundles (include/vrt_hip.h, vrt_hip_set_ray_index).  Key of a Gaussian: its centre quantised to 10 bits
// per axis over the bounding box of the finite centres (an axis of zero extent: 0), x in the lowest bit of every triple; a centre that is
// not finite: key 0.  Order: by key, ties by scene index -- a function of the scene alone, so a mirror's index is the same index.
// Sorted on the host from the rows read back: the caller has waited for everything in flight, as every table build does.
int build_ray_index(vrt_hip_ctx *c)
{
    const uint32_t n = c->n, nleaves = (n + 63u) / 64u, ngroups = (nleaves + 63u) / 64u;
    std::vector<float4> ms(n), gb(n), pms(n), pgb(n);
    if (n) {
        HIPCHK(c, hipMemcpy(ms.data(), c->mu_sig.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(gb.data(), c->gB.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    const std::vector<uint32_t> perm = morton_order(ms);
    for (uint32_t p = 0; p < n; ++p) { pms[p] = ms[perm[p]]; pgb[p] = gb[perm[p]]; }
    HIPCHK(c, c->ri_perm.reserve(n)); HIPCHK(c, c->ri_mu_sig.reserve(n)); HIPCHK(c, c->ri_gB.reserve(n));
    HIPCHK(c, c->ri_leaves.reserve(nleaves)); HIPCHK(c, c->ri_groups.reserve(ngroups));
    if (n) {
        HIPCHK(c, hipMemcpy(c->ri_perm.p, perm.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->ri_mu_sig.p, pms.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->ri_gB.p, pgb.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
    }
    // leaf spheres: the chunk table's arithmetic, margins included, over the permuted rows
    launch_build_chunks(n, c->ri_mu_sig.p, c->ri_gB.p, c->ri_leaves.p, c->stream);
    HIPCHK(c, hipGetLastError());
    // The chunk kernel's minima and maxima pass over a NaN: a member whose centre or reach is not finite would sit outside its leaf's
    // sphere, yet the member test keeps it (a comparison with NaN is false).  Such a leaf gets a NaN radius, which keeps.
    std::vector<uint32_t> open_leaves;
    for (uint32_t p = 0; p < n; ++p) {
        const bool ok = finite_centre(pms[p]) && !std::isnan(pgb[p].y) && !std::isnan(pgb[p].w) && pgb[p].w < INFINITY;
        if (!ok && (open_leaves.empty() || open_leaves.back() != p / 64u)) open_leaves.push_back(p / 64u);
    }
    if (!open_leaves.empty()) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const float nan = std::nanf("");
        for (uint32_t lf : open_leaves) HIPCHK(c, hipMemcpy(&c->ri_leaves.p[lf].w, &nan, sizeof(float), hipMemcpyHostToDevice));
    }
    launch_build_ray_groups(nleaves, c->ri_leaves.p, c->ri_groups.p, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream)); // bundles may use a caller's stream
    c->ray_index_dirty = false;
    return VRT_HIP_OK;
}

// The same index built on the device, behind the table build on `st` and with nothing waited for (vrt_scene_kernel.hip): serves a scene
// set from device memory.  A buffer that grows is freed first, which waits for the device -- a larger scene, the first build, more
// temporary storage for the sort; with the scene's size unchanged nothing waits.
int build_ray_index_device(vrt_hip_ctx *c, hipStream_t st)
{
    const uint32_t n = c->n, nleaves = (n + 63u) / 64u, ngroups = (nleaves + 63u) / 64u;
    if (c->ri_sort_n != n) {
        c->ri_sort_bytes = morton_sort_bytes(n);
        if (!c->ri_sort_bytes) return fail(c, VRT_HIP_ERR_HIP, "ray index: the sort's storage query failed");
        c->ri_sort_n = n;
    }
    HIPCHK(c, c->ri_perm.reserve(n)); HIPCHK(c, c->ri_mu_sig.reserve(n)); HIPCHK(c, c->ri_gB.reserve(n));
    HIPCHK(c, c->ri_leaves.reserve(nleaves)); HIPCHK(c, c->ri_groups.reserve(ngroups));
    HIPCHK(c, c->ri_keys.reserve((size_t)n * 2)); HIPCHK(c, c->ri_sort_tmp.reserve(c->ri_sort_bytes));
    HIPCHK(c, c->scene_words.reserve(8));
    HIPCHK(c, launch_morton_index(n, c->mu_sig.p, c->gB.p, c->iota.p, c->scene_words.p, c->ri_keys.p, c->ri_sort_tmp.p, c->ri_sort_bytes,
                                  c->ri_perm.p, c->ri_mu_sig.p, c->ri_gB.p, st));
    launch_build_chunks(n, c->ri_mu_sig.p, c->ri_gB.p, c->ri_leaves.p, st);
    launch_morton_open_leaves(n, c->ri_mu_sig.p, c->ri_gB.p, c->ri_leaves.p, st);
    launch_build_ray_groups(nleaves, c->ri_leaves.p, c->ri_groups.p, st);
    HIPCHK(c, hipGetLastError());
    c->ray_index_dirty = false;
    return VRT_HIP_OK;
}

namespace {

// A kind of bundle as its entry points see it: its name, what it calls its tables and results and their length in the messages, what
// its check asks on top of every kind's, and which kernels run.
struct BundleKind {
    const char *name, *io_text, *count;
    bool gradient; // a derivative: a scene of no Gaussians is a bundle of nothing, and the Exp / Erf pair must have kernels
    bool modes;    // ... of what `wrt` names
    void (*launch)(const RayArgs &, uint32_t, int, int, int, hipStream_t);
    // a gradient with the ordered switch on and a table (ordered_bundle): the kernels that record, whether a long ray files two records
    // per kept Gaussian, and the first column of the table its reduction writes
    void (*launch_ordered)(const RayArgs &, uint32_t, int, int, int, hipStream_t) = nullptr;
    bool ord_two = false;
    int ord_first_col = 0;
};
const BundleKind RADIANCE = { "radiance_rays", "no output buffer", "", false, false, launch_ray_bundle };
const BundleKind TRANSMITTANCE = { "transmittance_bundle", "NULL samples or result", "ns", false, false, launch_ray_trans_bundle };
const BundleKind DEPTH = { "depth_bundle", "NULL levels or result", "nt", false, false, launch_ray_depth_bundle };
const BundleKind GRADIENT = { "radiance_rays_grad", "NULL grad_radiance or gradient table", "", true, false, launch_ray_grad_bundle,
                              launch_ray_grad_bundle_ordered, true, 0 };
const BundleKind TRANS_GRADIENT = { "transmittance_bundle_grad", "NULL samples or grad_T, or neither a gradient table nor grad_s", "ns", true, true,
                                    launch_ray_trans_grad_bundle, launch_ray_trans_grad_bundle_ordered, false, 4 };
// the diagonal of J^T W J: a derivative; ordered, one record per (ray, kept Gaussian) in either kernel
const BundleKind GN_DIAG = { "radiance_rays_gn_diag", "NULL diagonal table", "", true, false, launch_ray_gn_diag_bundle, launch_ray_gn_diag_bundle_ordered,
                             false, 0 };
// forward mode: a derivative (the scene of no Gaussians, the pairs), but no table: nothing for the ordered switch to order
const BundleKind TANGENT = { "radiance_rays_tangent", "NULL output, or neither a tangent table nor ray tangents", "", true, false, launch_ray_tangent_bundle };
const BundleKind TRANS_TANGENT = { "transmittance_bundle_tangent", "NULL samples or output, or none of a tangent table, ray tangents and sample tangents", "ns",
                                   true, true, launch_ray_trans_tangent_bundle };

// The rays of a call, device or host pointers alike
struct Rays {
    size_t nrays;
    const float *origins;
    int origin_per_ray;
    const float *dirs;
};

// What a bound ray plan asks of a call, before anything is enqueued (include/vrt_hip.h, "Contract of a planned call")
int plan_admits(vrt_hip_ctx *c, const std::string &name, size_t nrays)
{
    const vrt_hip_ray_plan *p = c->plan;
    if (nrays != p->nrays)
        return fail(c, VRT_HIP_ERR_INVALID, name + ": the bound ray plan was made for " + std::to_string(p->nrays) + " rays, the call has " + std::to_string(nrays));
    if (c->plan_flags & VRT_HIP_PLAN_KEEP_LISTS) {
        if (c->n != p->scene_n)
            return fail(c, VRT_HIP_ERR_INVALID, name + ": the bound ray plan keeps lists of indices into a scene of " + std::to_string(p->scene_n) +
                                                    " Gaussians, the scene now has " + std::to_string(c->n));
    } else if (c->cull_gen != p->cull_gen)
        return fail(c, VRT_HIP_ERR_INVALID, name + ": the bound ray plan is stale: " + c->cull_gen_why +
                                                " after it was made (make it again, or bind it with VRT_HIP_PLAN_KEEP_LISTS to hold its lists)");
    return VRT_HIP_OK;
}

// What every entry point checks before anything else, host and device form alike.  n: values per ray (1 for radiance and its gradient);
// io_ok: the kind's tables and results are there; wrt: read by a kind with modes only.  True when the call is over, with rc its result:
// an error, or VRT_HIP_OK for a bundle of nothing.
bool bundle_over(vrt_hip_ctx *c, const BundleKind &k, const Rays &r, size_t n, bool io_ok, int wrt, int &rc)
{
    const std::string name = k.name;
    if (!c) rc = VRT_HIP_ERR_INVALID;
    else if (c->plan && (rc = plan_admits(c, name, r.nrays)) != VRT_HIP_OK) {} // before anything else: a planned call states its plan's rays
    else if (r.nrays == 0 || n == 0 || (k.gradient && c->n == 0)) rc = VRT_HIP_OK;
    else if (!r.origins || !r.dirs) rc = fail(c, VRT_HIP_ERR_INVALID, name + ": NULL origins or directions");
    else if (!io_ok) rc = fail(c, VRT_HIP_ERR_INVALID, name + ": " + k.io_text);
    else if (r.nrays > 0xFFFFFFF0ull) rc = fail(c, VRT_HIP_ERR_INVALID, name + ": more than 2^32 - 16 rays in one bundle");
    else if (n > (SIZE_MAX / sizeof(float)) / r.nrays) rc = fail(c, VRT_HIP_ERR_INVALID, name + ": nrays * " + k.count + " does not fit");
    else if (k.gradient && !ray_grad_pair_supported(c->exp_kind, c->erf_kind))
        rc = fail(c, VRT_HIP_ERR_INVALID, name + ": the derivative is taken under {vcl_exp, expf} x {A&S erf, erff} only; the selected pair has jumps");
    else if (k.modes && wrt != VRT_HIP_TGRAD_T && wrt != VRT_HIP_TGRAD_DEPTH)
        rc = fail(c, VRT_HIP_ERR_INVALID, name + ": wrt is neither VRT_HIP_TGRAD_T nor VRT_HIP_TGRAD_DEPTH");
    else return false;
    return true;
}

// A gradient bundle with a table while vrt_hip_set_grad_ordered is on (include/vrt_hip.h has the contract, vrt_grad_ordered_kernel.hip
// the pipeline): count and place, ONE wait for the total, then the record kernels, the sort and the reduction -- or, where no ray keeps
// anything, the kernels of the switch off, which then add nothing.  Refused before anything touches the table: a total beyond 2^32 - 1,
// a buffer that cannot grow.
int ordered_bundle(vrt_hip_ctx *c, const BundleKind &k, Bundle &b, hipStream_t st)
{
    RayArgs &a = b.a;
    const size_t nrays = (size_t)a.nrays;
    const size_t scan_bytes = grad_ordered_scan_bytes(nrays);
    if (!scan_bytes) return fail(c, VRT_HIP_ERR_HIP, std::string(k.name) + ": ordered table: the scan's storage query failed");
    HIPCHK(c, c->ord_len.reserve(nrays)); HIPCHK(c, c->ord_count.reserve(nrays)); HIPCHK(c, c->ord_base.reserve(nrays));
    HIPCHK(c, c->ord_words.reserve(GRAD_ORD_WORDS)); HIPCHK(c, c->ord_scan_tmp.reserve(scan_bytes));
    a.ord_len = c->ord_len.p; a.ord_count = c->ord_count.p; a.ord_two = k.ord_two ? 1 : 0; a.ord_base = c->ord_base.p;
    a.ord_words = c->ord_words.p;
    c->ord_valid = true; c->ord_total = 0;
    HIPCHK(c, launch_grad_ordered_count(a, b.src, c->ord_base.p, c->ord_scan_tmp.p, scan_bytes, st));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, c->ord_words.p + GRAD_ORD_TOTAL, sizeof(total), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st)); // the one wait of an ordered call: the sort takes its size on the host, and the buffers may have to grow
    if (total > 0xFFFFFFFFull) return fail(c, VRT_HIP_ERR_INVALID, std::string(k.name) + ": ordered table: more than 2^32 - 1 records in one bundle");
    if (total == 0) { // no ray keeps anything: nothing to record, sort or reduce; ray rows, grad_s and statistics by the kernels of the switch off
        k.launch(a, b.grid, b.src, c->exp_kind, c->erf_kind, st);
        HIPCHK(c, hipGetLastError());
        return VRT_HIP_OK;
    }
    const size_t rows = (size_t)total;
    const size_t sort_bytes = grad_ordered_sort_bytes(total, c->n);
    if (!sort_bytes) return fail(c, VRT_HIP_ERR_HIP, std::string(k.name) + ": ordered table: the sort's storage query failed");
    HIPCHK(c, c->ord_gauss.reserve(rows)); HIPCHK(c, c->ord_ray.reserve(rows)); HIPCHK(c, c->ord_rows.reserve(rows * GRAD_ORD_COLS));
    HIPCHK(c, c->ord_keys_sorted.reserve(rows)); HIPCHK(c, c->ord_order.reserve(rows)); HIPCHK(c, c->ord_seg.reserve((size_t)c->n * 2));
    HIPCHK(c, c->ord_sort_tmp.reserve(sort_bytes));
    if (c->ord_iota.cap < rows) { c->ord_iota_filled = 0; HIPCHK(c, c->ord_iota.reserve(rows)); }
    if (c->ord_iota_filled < rows) {
        launch_grad_ordered_iota(c->ord_iota.p, c->ord_iota_filled, rows, st);
        c->ord_iota_filled = rows;
    }
    a.ord_gauss = c->ord_gauss.p; a.ord_ray = c->ord_ray.p; a.ord_rows = c->ord_rows.p;
    k.launch_ordered(a, b.grid, b.src, c->exp_kind, c->erf_kind, st);
    HIPCHK(c, hipGetLastError());
    GradOrderedSort o{};
    o.total = total; o.n = c->n;
    o.keys = c->ord_gauss.p; o.iota = c->ord_iota.p; o.keys_sorted = c->ord_keys_sorted.p; o.order = c->ord_order.p; o.seg = c->ord_seg.p;
    o.sort_tmp = c->ord_sort_tmp.p; o.sort_bytes = sort_bytes;
    o.rows = c->ord_rows.p; o.table = a.grad; o.first_col = k.ord_first_col; o.words = c->ord_words.p;
    HIPCHK(c, launch_grad_ordered_reduce(o, st));
    c->ord_total = total; c->ord_ran = true;
    return VRT_HIP_OK;
}

// The device form of every kind: the check, what the kind reserves of its own behind it (reserve: an error ends the call), what every
// bundle enqueues, the kind's own fields of RayArgs (fill), its two kernels
template <class Fill, class Reserve>
int device_bundle(vrt_hip_ctx *c, const BundleKind &k, const Rays &r, size_t n, bool io_ok, int wrt, void *hip_stream, Fill &&fill, Reserve &&reserve)
{
    int rc;
    if (bundle_over(c, k, r, n, io_ok, wrt, rc)) return rc;
    if ((rc = reserve()) != VRT_HIP_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    Bundle b;
    rc = enqueue_bundle(c, r.nrays, r.origins, r.origin_per_ray, r.dirs, st, b);
    if (rc) return rc;
    fill(b.a);
    if (c->grad_ordered && k.launch_ordered && b.a.grad) return ordered_bundle(c, k, b, st);
    k.launch(b.a, b.grid, b.src, c->exp_kind, c->erf_kind, st);
    HIPCHK(c, hipGetLastError());
    return VRT_HIP_OK;
}

template <class Fill>
int device_bundle(vrt_hip_ctx *c, const BundleKind &k, const Rays &r, size_t n, bool io_ok, int wrt, void *hip_stream, Fill &&fill)
{
    return device_bundle(c, k, r, n, io_ok, wrt, hip_stream, fill, [] { return (int)VRT_HIP_OK; });
}

// A staging buffer of any element type, as the host path sees it: the path moves bytes
struct AnyBuf {
    void *buf;
    size_t size; // of one element
    hipError_t (*reserve_fn)(void *, size_t);
    void *(*data_fn)(void *);
    template <typename T>
    AnyBuf(DevBuf<T> &b)
        : buf(&b), size(sizeof(T)), reserve_fn([](void *p, size_t n) { return ((DevBuf<T> *)p)->reserve(n); }),
          data_fn([](void *p) -> void * { return ((DevBuf<T> *)p)->p; })
    {
    }
    hipError_t reserve(size_t n) const { return reserve_fn(buf, n); }
    void *data() const { return data_fn(buf); }
};
// What a host-pointer form states: `count` elements at `host` copied into a staging buffer ahead of the device form ...
struct CopiedIn {
    AnyBuf buf;
    const void *host;
    size_t count;
};
// ... and `count` elements brought back from one behind it, the buffer cleared first where the kernels add to it.  A result the caller
// did not ask for (host == nullptr) is left out altogether.
struct BroughtBack {
    AnyBuf buf;
    void *host;
    size_t count;
    bool clear = false;
};

// The host-pointer form of every kind, behind its check (the lists name buffers of *c): nothing in flight (an earlier bundle may still
// read the staging buffers), every reservation before any copy (no buffer grows behind a copy), rays and `in` copied in, the results
// that ask for it cleared, the device form on the context's stream over the staging buffers, `out` copied back and waited for.
template <class Device>
int host_bundle(vrt_hip_ctx *c, const Rays &r, std::initializer_list<CopiedIn> in, std::initializer_list<BroughtBack> out, Device &&device)
{
    HIPCHK(c, hipSetDevice(c->device));
    int rc = quiesce(c);
    if (rc) return rc;
    const size_t no = (r.origin_per_ray ? r.nrays : 1) * 3;
    for (const CopiedIn &s : in)
        if (s.host) HIPCHK(c, s.buf.reserve(s.count)); // (an input the kind lets the caller leave out: host == nullptr)
    for (const BroughtBack &s : out)
        if (s.host) HIPCHK(c, s.buf.reserve(s.count));
    HIPCHK(c, c->rays_in[0].reserve(no));
    HIPCHK(c, c->rays_in[1].reserve(r.nrays * 3));
    HIPCHK(c, hipMemcpyAsync(c->rays_in[0].p, r.origins, no * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rays_in[1].p, r.dirs, r.nrays * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    for (const CopiedIn &s : in)
        if (s.host) HIPCHK(c, hipMemcpyAsync(s.buf.data(), s.host, s.count * s.buf.size, hipMemcpyHostToDevice, c->stream));
    for (const BroughtBack &s : out)
        if (s.host && s.clear) HIPCHK(c, hipMemsetAsync(s.buf.data(), 0, s.count * s.buf.size, c->stream));
    c->ord_ran = false;
    rc = device(Rays{ r.nrays, c->rays_in[0].p, r.origin_per_ray, c->rays_in[1].p });
    if (rc) return rc;
    for (const BroughtBack &s : out)
        if (s.host) HIPCHK(c, hipMemcpyAsync(s.host, s.buf.data(), s.count * s.buf.size, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->ord_ran) { // an ordered table: a ray that missed its counted length filed nothing, and the table is short of it
        unsigned long long missed = 0;
        HIPCHK(c, hipMemcpy(&missed, c->ord_words.p + GRAD_ORD_MISMATCH, sizeof(missed), hipMemcpyDeviceToHost));
        if (missed) return fail(c, VRT_HIP_ERR_HIP, "ordered table: " + std::to_string(missed) + " rays missed the list length the count pass found");
    }
    return VRT_HIP_OK;
}

// the staging buffer of a result, or nullptr where the caller did not ask for that result
template <typename T>
T *wanted(const void *host, const DevBuf<T> &b) { return host ? b.p : nullptr; }

} // namespace

extern "C" {

int vrt_hip_radiance_rays_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                 float *d_radiance, uint32_t *d_image, int pack_flags, void *hip_stream)
{
    return device_bundle(c, RADIANCE, { nrays, d_origins, origin_per_ray, d_dirs }, 1, d_radiance || d_image, 0, hip_stream, [&](RayArgs &a) {
        a.radiance = (float4 *)d_radiance; a.image = d_image; a.pack_flags = pack_flags;
    });
}

int vrt_hip_radiance_rays(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                          float *radiance_out, uint32_t *image_out, int pack_flags)
{
    const Rays r = { nrays, origins, origin_per_ray, dirs };
    int rc;
    if (bundle_over(c, RADIANCE, r, 1, radiance_out || image_out, 0, rc)) return rc;
    return host_bundle(c, r, {},
                       { { c->rays_rad, radiance_out, nrays }, { c->rays_img, image_out, nrays } }, [&](const Rays &d) {
                           return vrt_hip_radiance_rays_device(c, d.nrays, d.origins, d.origin_per_ray, d.dirs, (float *)wanted(radiance_out, c->rays_rad),
                                                               wanted(image_out, c->rays_img), pack_flags, c->stream);
                       });
}

int vrt_hip_radiance_rays_grad_rays_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                           const float *d_grad_radiance, float *d_grad, float *d_grad_rays, void *hip_stream)
{
    return device_bundle(c, GRADIENT, { nrays, d_origins, origin_per_ray, d_dirs }, 1, d_grad_radiance && (d_grad || d_grad_rays), 0, hip_stream,
                         [&](RayArgs &a) {
                             a.grad_radiance = (const float4 *)d_grad_radiance; a.grad = d_grad; a.grad_rays = d_grad_rays;
                         });
}

// grad_radiance in; a cleared table of the scene's size and the ray rows out, either where asked for
int vrt_hip_radiance_rays_grad_rays(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                                    const float *grad_radiance, float *grad_out, float *grad_rays_out)
{
    const Rays r = { nrays, origins, origin_per_ray, dirs };
    int rc;
    if (bundle_over(c, GRADIENT, r, 1, grad_radiance && (grad_out || grad_rays_out), 0, rc)) return rc;
    return host_bundle(c, r, { { c->rays_each_in, grad_radiance, nrays * 4 } },
                       { { c->rays_table_out, grad_out, (size_t)c->n * VRT_HIP_GRAD_STRIDE, true },
                         { c->rays_rows_out, grad_rays_out, nrays * VRT_HIP_RAY_GRAD_STRIDE } },
                       [&](const Rays &d) {
                           return vrt_hip_radiance_rays_grad_rays_device(c, d.nrays, d.origins, d.origin_per_ray, d.dirs, c->rays_each_in.p,
                                                                         wanted(grad_out, c->rays_table_out), wanted(grad_rays_out, c->rays_rows_out),
                                                                         c->stream);
                       });
}

// the table alone: the same calls without the ray rows
int vrt_hip_radiance_rays_grad_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                      const float *d_grad_radiance, float *d_grad, void *hip_stream)
{
    return vrt_hip_radiance_rays_grad_rays_device(c, nrays, d_origins, origin_per_ray, d_dirs, d_grad_radiance, d_grad, nullptr, hip_stream);
}

int vrt_hip_radiance_rays_grad(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                               const float *grad_radiance, float *grad_out)
{
    return vrt_hip_radiance_rays_grad_rays(c, nrays, origins, origin_per_ray, dirs, grad_radiance, grad_out, nullptr);
}

// The workspace of the diagonal's long kernel: a list position from RAY_LCAP on keeps its GN_SUMS running sums in device memory, in the
// slot of its workgroup -- GN_SUMS * 4 bytes per Gaussian beyond RAY_LCAP.  The slots stay within 256 MB, which caps the long kernel's
// grid -- never below one workgroup, whose single slot is reserved in full even where it alone passes 256 MB (N above 5.6 M); a
// scene of at most RAY_LCAP Gaussians has no workspace.  Grows only, like the scratch slots.
static int gn_diag_workspace(vrt_hip_ctx *c, uint64_t &slot, uint32_t &grid)
{
    grid = long_grid(c);
    slot = c->n > (uint32_t)RAY_LCAP ? (uint64_t)(c->n - (uint32_t)RAY_LCAP) * GN_SUMS : 0;
    if (!slot) return VRT_HIP_OK;
    const uint64_t by_memory = ((uint64_t)256 << 20) / (slot * sizeof(float));
    grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(grid, by_memory));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->gn_work.reserve((size_t)slot * grid)); // (a buffer that grows is freed first, which waits for the device)
    return VRT_HIP_OK;
}

// weights in (or none); the diagonal ADDED into the caller's table
int vrt_hip_radiance_rays_gn_diag_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                         const float *d_weights, float *d_diag, void *hip_stream)
{
    uint64_t slot = 0;
    uint32_t grid = 0;
    return device_bundle(c, GN_DIAG, { nrays, d_origins, origin_per_ray, d_dirs }, 1, d_diag != nullptr, 0, hip_stream, [&](RayArgs &a) {
        a.gn_weights = (const float4 *)d_weights; a.grad = d_diag;
        a.gn_work = c->gn_work.p; a.gn_work_slot = slot; a.gn_grid = grid;
    }, [&] { return gn_diag_workspace(c, slot, grid); });
}

// a cleared table of the scene's size out
int vrt_hip_radiance_rays_gn_diag(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs, const float *weights,
                                  float *diag_out)
{
    const Rays r = { nrays, origins, origin_per_ray, dirs };
    int rc;
    if (bundle_over(c, GN_DIAG, r, 1, diag_out != nullptr, 0, rc)) return rc;
    return host_bundle(c, r, { { c->rays_each_in, weights, nrays * 4 } }, { { c->rays_table_out, diag_out, (size_t)c->n * VRT_HIP_GRAD_STRIDE, true } },
                       [&](const Rays &d) {
                           return vrt_hip_radiance_rays_gn_diag_device(c, d.nrays, d.origins, d.origin_per_ray, d.dirs, wanted(weights, c->rays_each_in),
                                                                       c->rays_table_out.p, c->stream);
                       });
}

// forward mode: the direction in, J . v of the radiance out
int vrt_hip_radiance_rays_tangent_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                         const float *d_tangent, const float *d_ray_tangent, float *d_out, void *hip_stream)
{
    return device_bundle(c, TANGENT, { nrays, d_origins, origin_per_ray, d_dirs }, 1, d_out && (d_tangent || d_ray_tangent), 0, hip_stream,
                         [&](RayArgs &a) {
                             a.tangent = d_tangent; a.ray_tangent = d_ray_tangent; a.tangent_out = (float4 *)d_out;
                         });
}

// the tangent table of the scene's size and the ray tangents in, either where given; 4 floats per ray out
int vrt_hip_radiance_rays_tangent(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs, const float *tangent,
                                  const float *ray_tangent, float *out)
{
    const Rays r = { nrays, origins, origin_per_ray, dirs };
    int rc;
    if (bundle_over(c, TANGENT, r, 1, out && (tangent || ray_tangent), 0, rc)) return rc;
    return host_bundle(c, r, { { c->rays_table_in, tangent, (size_t)c->n * VRT_HIP_GRAD_STRIDE },
                               { c->rays_rows_in, ray_tangent, nrays * VRT_HIP_RAY_GRAD_STRIDE } },
                       { { c->rays_rad, out, nrays } }, [&](const Rays &d) {
                           return vrt_hip_radiance_rays_tangent_device(c, d.nrays, d.origins, d.origin_per_ray, d.dirs, wanted(tangent, c->rays_table_in),
                                                                       wanted(ray_tangent, c->rays_rows_in), (float *)c->rays_rad.p, c->stream);
                       });
}

// what the two forms of the transmittance tangent bundle check: every kind's, and that depth mode has a depth per ray
static bool trans_tangent_over(vrt_hip_ctx *c, const Rays &r, size_t ns, int s_per_ray, bool io_ok, int wrt, int &rc)
{
    if (bundle_over(c, TRANS_TANGENT, r, ns, io_ok, wrt, rc)) return true;
    if (wrt == VRT_HIP_TGRAD_DEPTH && !s_per_ray) {
        rc = fail(c, VRT_HIP_ERR_INVALID, std::string(TRANS_TANGENT.name) + ": depth mode takes the depths of every ray (s_per_ray == 0)");
        return true;
    }
    return false;
}

// forward mode: the direction in, J . v of the transmittance (or of the depth) out
int vrt_hip_transmittance_bundle_tangent_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                                const float *d_s, size_t ns, int s_per_ray, int wrt, const float *d_tangent,
                                                const float *d_ray_tangent, const float *d_s_tangent, int s_tangent_per_ray, float *d_out,
                                                void *hip_stream)
{
    const Rays r = { nrays, d_origins, origin_per_ray, d_dirs };
    const bool io_ok = d_s && d_out && (d_tangent || d_ray_tangent || d_s_tangent);
    int rc;
    if (trans_tangent_over(c, r, ns, s_per_ray, io_ok, wrt, rc)) return rc;
    return device_bundle(c, TRANS_TANGENT, r, ns, io_ok, wrt, hip_stream, [&](RayArgs &a) {
        a.s = d_s; a.ns = ns; a.s_per_ray = s_per_ray ? 1 : 0; a.wrt = wrt;
        a.tangent = d_tangent; a.ray_tangent = d_ray_tangent;
        a.s_tangent = d_s_tangent; a.s_tangent_per_ray = s_tangent_per_ray ? 1 : 0; a.trans_tangent_out = d_out;
    });
}

// samples, the tangent table of the scene's size, the ray tangents and the sample tangents in, each of the three where given; a float per ray and sample out
int vrt_hip_transmittance_bundle_tangent(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs, const float *s,
                                         size_t ns, int s_per_ray, int wrt, const float *tangent, const float *ray_tangent, const float *s_tangent,
                                         int s_tangent_per_ray, float *out)
{
    const Rays r = { nrays, origins, origin_per_ray, dirs };
    int rc;
    if (trans_tangent_over(c, r, ns, s_per_ray, s && out && (tangent || ray_tangent || s_tangent), wrt, rc)) return rc;
    return host_bundle(c, r, { { c->rays_values_in, s, (s_per_ray ? nrays : 1) * ns },
                               { c->rays_table_in, tangent, (size_t)c->n * VRT_HIP_GRAD_STRIDE },
                               { c->rays_rows_in, ray_tangent, nrays * VRT_HIP_RAY_GRAD_STRIDE },
                               { c->rays_each_in, s_tangent, (s_tangent_per_ray ? nrays : 1) * ns } },
                       { { c->rays_each_out, out, nrays * ns } }, [&](const Rays &d) {
                           return vrt_hip_transmittance_bundle_tangent_device(c, d.nrays, d.origins, d.origin_per_ray, d.dirs, c->rays_values_in.p, ns,
                                                                              s_per_ray, wrt, wanted(tangent, c->rays_table_in),
                                                                              wanted(ray_tangent, c->rays_rows_in), wanted(s_tangent, c->rays_each_in),
                                                                              s_tangent_per_ray, c->rays_each_out.p, c->stream);
                       });
}

int vrt_hip_transmittance_bundle_grad_rays_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                                  const float *d_s, size_t ns, int s_per_ray, const float *d_grad_T, int wrt, float *d_grad,
                                                  float *d_grad_s, float *d_grad_rays, void *hip_stream)
{
    return device_bundle(c, TRANS_GRADIENT, { nrays, d_origins, origin_per_ray, d_dirs }, ns, d_s && d_grad_T && (d_grad || d_grad_s || d_grad_rays), wrt,
                         hip_stream, [&](RayArgs &a) {
                             a.s = d_s; a.ns = ns; a.s_per_ray = s_per_ray ? 1 : 0;
                             a.grad_T = d_grad_T; a.wrt = wrt; a.grad = d_grad; a.grad_s = d_grad_s; a.grad_rays = d_grad_rays;
                         });
}

// samples and grad_T in; a cleared table of the scene's size, the per-sample output and the ray rows out, each where asked for
int vrt_hip_transmittance_bundle_grad_rays(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs, const float *s,
                                           size_t ns, int s_per_ray, const float *grad_T, int wrt, float *grad_out, float *grad_s_out,
                                           float *grad_rays_out)
{
    const Rays r = { nrays, origins, origin_per_ray, dirs };
    int rc;
    if (bundle_over(c, TRANS_GRADIENT, r, ns, s && grad_T && (grad_out || grad_s_out || grad_rays_out), wrt, rc)) return rc;
    return host_bundle(c, r, { { c->rays_values_in, s, (s_per_ray ? nrays : 1) * ns }, { c->rays_each_in, grad_T, nrays * ns } },
                       { { c->rays_table_out, grad_out, (size_t)c->n * VRT_HIP_GRAD_STRIDE, true },
                         { c->rays_each_out, grad_s_out, nrays * ns },
                         { c->rays_rows_out, grad_rays_out, nrays * VRT_HIP_RAY_GRAD_STRIDE } },
                       [&](const Rays &d) {
                           return vrt_hip_transmittance_bundle_grad_rays_device(c, d.nrays, d.origins, d.origin_per_ray, d.dirs, c->rays_values_in.p, ns,
                                                                                s_per_ray, c->rays_each_in.p, wrt, wanted(grad_out, c->rays_table_out),
                                                                                wanted(grad_s_out, c->rays_each_out),
                                                                                wanted(grad_rays_out, c->rays_rows_out), c->stream);
                       });
}

int vrt_hip_transmittance_bundle_grad_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                             const float *d_s, size_t ns, int s_per_ray, const float *d_grad_T, int wrt, float *d_grad, float *d_grad_s,
                                             void *hip_stream)
{
    return vrt_hip_transmittance_bundle_grad_rays_device(c, nrays, d_origins, origin_per_ray, d_dirs, d_s, ns, s_per_ray, d_grad_T, wrt, d_grad, d_grad_s,
                                                         nullptr, hip_stream);
}

int vrt_hip_transmittance_bundle_grad(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs, const float *s,
                                      size_t ns, int s_per_ray, const float *grad_T, int wrt, float *grad_out, float *grad_s_out)
{
    return vrt_hip_transmittance_bundle_grad_rays(c, nrays, origins, origin_per_ray, dirs, s, ns, s_per_ray, grad_T, wrt, grad_out, grad_s_out, nullptr);
}

int vrt_hip_transmittance_bundle_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                        const float *d_s, size_t ns, int s_per_ray, float *d_T, void *hip_stream)
{
    return device_bundle(c, TRANSMITTANCE, { nrays, d_origins, origin_per_ray, d_dirs }, ns, d_s && d_T, 0, hip_stream, [&](RayArgs &a) {
        a.s = d_s; a.ns = ns; a.s_per_ray = s_per_ray ? 1 : 0; a.T = d_T;
    });
}

// sample distances in; T per ray and sample out
int vrt_hip_transmittance_bundle(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs, const float *s,
                                 size_t ns, int s_per_ray, float *T_out)
{
    const Rays r = { nrays, origins, origin_per_ray, dirs };
    int rc;
    if (bundle_over(c, TRANSMITTANCE, r, ns, s && T_out, 0, rc)) return rc;
    return host_bundle(c, r, { { c->rays_values_in, s, (s_per_ray ? nrays : 1) * ns } },
                       { { c->rays_each_out, T_out, nrays * ns } }, [&](const Rays &d) {
                           return vrt_hip_transmittance_bundle_device(c, d.nrays, d.origins, d.origin_per_ray, d.dirs, c->rays_values_in.p, ns, s_per_ray,
                                                                      c->rays_each_out.p, c->stream);
                       });
}

int vrt_hip_depth_bundle_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs, const float *d_tau,
                                size_t nt, int tau_per_ray, float *d_depth, void *hip_stream)
{
    return device_bundle(c, DEPTH, { nrays, d_origins, origin_per_ray, d_dirs }, nt, d_tau && d_depth, 0, hip_stream, [&](RayArgs &a) {
        a.tau = d_tau; a.nt = nt; a.tau_per_ray = tau_per_ray ? 1 : 0; a.depth = d_depth;
    });
}

// levels in; the depth per ray and level out
int vrt_hip_depth_bundle(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs, const float *tau, size_t nt,
                         int tau_per_ray, float *depth_out)
{
    const Rays r = { nrays, origins, origin_per_ray, dirs };
    int rc;
    if (bundle_over(c, DEPTH, r, nt, tau && depth_out, 0, rc)) return rc;
    return host_bundle(c, r, { { c->rays_values_in, tau, (tau_per_ray ? nrays : 1) * nt } },
                       { { c->rays_each_out, depth_out, nrays * nt } }, [&](const Rays &d) {
                           return vrt_hip_depth_bundle_device(c, d.nrays, d.origins, d.origin_per_ray, d.dirs, c->rays_values_in.p, nt, tau_per_ray, c->rays_each_out.p,
                                                              c->stream);
                       });
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

int vrt_hip_get_grad_ordered_stats(vrt_hip_ctx *c, vrt_hip_grad_ordered_stats *out)
{
    if (!c || !out) return VRT_HIP_ERR_INVALID;
    *out = vrt_hip_grad_ordered_stats{};
    if (!c->ord_valid) return VRT_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // waits for the call
    unsigned long long w[GRAD_ORD_WORDS];
    HIPCHK(c, hipMemcpy(w, c->ord_words.p, sizeof(w), hipMemcpyDeviceToHost));
    out->records = w[GRAD_ORD_RECORDS]; out->gaussians = w[GRAD_ORD_TOUCHED]; out->longest = w[GRAD_ORD_LONGEST]; out->mismatches = w[GRAD_ORD_MISMATCH];
    return VRT_HIP_OK;
}

// The records as the reduction consumed them: the sorted keys and the order are the sort's; sentinel rows sort last, so the first
// `records` places of the order are the records.  Gathered on the host: a read-out, not a hot path.
int vrt_hip_get_grad_records(vrt_hip_ctx *c, uint32_t *gauss, uint32_t *ray, float *rows, size_t cap, size_t *count)
{
    if (!c || !count) return VRT_HIP_ERR_INVALID;
    *count = 0;
    if (!c->ord_valid || !c->ord_total) return VRT_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // waits for the call
    unsigned long long w[GRAD_ORD_WORDS];
    HIPCHK(c, hipMemcpy(w, c->ord_words.p, sizeof(w), hipMemcpyDeviceToHost));
    const size_t n = (size_t)w[GRAD_ORD_RECORDS], total = (size_t)c->ord_total;
    *count = n;
    if (n > cap || (n && (!gauss || !ray || !rows))) return fail(c, VRT_HIP_ERR_INVALID, "get_grad_records: buffer too small");
    if (!n) return VRT_HIP_OK;
    std::vector<uint32_t> order(n), rays(total);
    std::vector<float> all(total * GRAD_ORD_COLS);
    HIPCHK(c, hipMemcpy(gauss, c->ord_keys_sorted.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(order.data(), c->ord_order.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(rays.data(), c->ord_ray.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(all.data(), c->ord_rows.p, total * GRAD_ORD_COLS * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        ray[i] = rays[order[i]];
        std::memcpy(rows + i * GRAD_ORD_COLS, all.data() + (size_t)order[i] * GRAD_ORD_COLS, GRAD_ORD_COLS * sizeof(float));
    }
    return VRT_HIP_OK;
}

int vrt_hip_get_ray_index_stats(vrt_hip_ctx *c, vrt_hip_ray_index_stats *out)
{
    if (!c || !out) return VRT_HIP_ERR_INVALID;
    *out = vrt_hip_ray_index_stats{};
    if (!c->ray_stats_valid || !c->ray_indexed_last) return VRT_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // waits for the bundle
    unsigned long long w[RAY_INDEX_STATS_WORDS];
    HIPCHK(c, hipMemcpy(w, c->ray_stats.p + RAY_STATS_WORDS, sizeof(w), hipMemcpyDeviceToHost));
    out->indexed = 1; out->groups = c->ri_last_groups; out->leaves = c->ri_last_leaves;
    out->groups_tested = w[0]; out->groups_kept = w[1]; out->leaves_tested = w[2]; out->leaves_kept = w[3]; out->members_tested = w[4];
    return VRT_HIP_OK;
}

int vrt_hip_get_ray_sort_stats(vrt_hip_ctx *c, vrt_hip_ray_sort_stats *out)
{
    if (!c || !out) return VRT_HIP_ERR_INVALID;
    *out = vrt_hip_ray_sort_stats{};
    if (!c->rs_last_valid) return VRT_HIP_OK;
    out->rays = c->rs_last_rays;
    if (!c->rs_last_sorted) return VRT_HIP_OK;
    if (c->rs_last_plan) { out->sorted = 1; return VRT_HIP_OK; } // a planned bundle in its plan's order; the plan keeps no count of the rays without sphere
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // waits for the bundle
    unsigned long long none = 0;
    HIPCHK(c, hipMemcpy(&none, c->rs_none.p, sizeof(none), hipMemcpyDeviceToHost));
    out->sorted = 1; out->rays_without_sphere = none;
    return VRT_HIP_OK;
}

int vrt_hip_get_ray_order(vrt_hip_ctx *c, uint32_t *order, uint32_t *keys, size_t cap, size_t *count)
{
    if (!c || !count) return VRT_HIP_ERR_INVALID;
    *count = 0;
    const vrt_hip_ray_plan *plan = c->rs_last_valid ? c->rs_last_plan : nullptr; // a planned bundle: its plan's order, whatever the switch says
    if ((!c->ray_sort && !plan) || !c->rs_last_valid || !c->rs_last_sorted)
        return fail(c, VRT_HIP_ERR_INVALID, "get_ray_order: the sort is off, or the last bundle was not sorted");
    const size_t n = c->rs_last_rays;
    *count = n;
    if (!order || cap < n) return fail(c, VRT_HIP_ERR_INVALID, "get_ray_order: buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // waits for the bundle
    HIPCHK(c, hipMemcpy(order, plan ? plan->order.p : c->rs_order.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (keys) { // filed packed: the documented key back
        HIPCHK(c, hipMemcpy(keys, plan ? plan->keys.p : c->rs_keys.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < n; ++r) keys[r] = ray_sort_unpack(keys[r], c->rs_last_spheres);
    }
    return VRT_HIP_OK;
}

// ---- ray plans (include/vrt_hip.h has the contract, vrt_ray_plan_kernel.hip the kernels) ----
static bool plan_of(const vrt_hip_ctx *c, const vrt_hip_ray_plan *plan)
{
    return plan && std::find(c->plans.begin(), c->plans.end(), plan) != c->plans.end();
}

// Count, scan, ONE wait for the totals, fill, and the wait that makes the plan complete.  The cull is the unplanned bundle's: whatever
// plan is bound stays out of it.  The statistics words are left alone (a creation is no bundle: vrt_hip_get_ray_stats reads zeros behind it).
int vrt_hip_ray_plan_create_device(vrt_hip_ctx *c, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs, void *hip_stream,
                                   vrt_hip_ray_plan **out)
{
    if (!c || !out) return VRT_HIP_ERR_INVALID;
    *out = nullptr;
    if (nrays && (!d_origins || !d_dirs)) return fail(c, VRT_HIP_ERR_INVALID, "ray_plan_create: NULL origins or directions");
    if (nrays > 0xFFFFFFF0ull) return fail(c, VRT_HIP_ERR_INVALID, "ray_plan_create: more than 2^32 - 16 rays in one plan");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    std::unique_ptr<vrt_hip_ray_plan> plan(new vrt_hip_ray_plan);
    plan->owner = c; plan->nrays = nrays;
    if (nrays) {
        Bundle b;
        vrt_hip_ray_plan *bound = c->plan;
        c->plan = nullptr;
        const int rc = enqueue_bundle(c, nrays, d_origins, origin_per_ray, d_dirs, st, b);
        c->plan = bound;
        if (rc) return rc;
        RayArgs &a = b.a;
        a.stats = nullptr; a.index_stats = nullptr;
        c->ray_stats_valid = false;
        plan->indexed = b.src == RAY_LIST_INDEX;
        plan->sorted = a.order != nullptr;
        // what only the creation needs: the scan's input and storage, the words
        DevBuf<unsigned long long> count, words;
        DevBuf<unsigned char> scan_tmp;
        const size_t scan_bytes = grad_ordered_scan_bytes(nrays);
        if (!scan_bytes) return fail(c, VRT_HIP_ERR_HIP, "ray_plan_create: the scan's storage query failed");
        HIPCHK(c, plan->len.reserve(nrays)); HIPCHK(c, plan->off.reserve(nrays + 1));
        HIPCHK(c, count.reserve(nrays)); HIPCHK(c, words.reserve(RAY_PLAN_WORDS)); HIPCHK(c, scan_tmp.reserve(scan_bytes));
        a.ord_len = plan->len.p; a.ord_count = count.p; a.ord_two = 0; a.ord_words = words.p;
        HIPCHK(c, launch_grad_ordered_count(a, b.src, plan->off.p, scan_tmp.p, scan_bytes, st));
        HIPCHK(c, launch_ray_plan_info(plan->len.p, nrays, words.p, st));
        unsigned long long w[RAY_PLAN_WORDS] = {};
        HIPCHK(c, hipMemcpyAsync(w, words.p, sizeof(w), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st)); // the lists and the queue take their size on the host
        const unsigned long long total = w[GRAD_ORD_TOTAL];
        if (total > 0xFFFFFFFFull) return fail(c, VRT_HIP_ERR_INVALID, "ray_plan_create: more than 2^32 - 1 kept entries in one plan");
        plan->entries = total; plan->long_rays = w[RAY_PLAN_LONG]; plan->scratch_rays = w[RAY_PLAN_SCRATCH]; plan->longest = w[RAY_PLAN_LONGEST];
        HIPCHK(c, plan->list.reserve((size_t)total)); HIPCHK(c, plan->long_ids.reserve((size_t)plan->long_rays));
        HIPCHK(c, hipMemcpyAsync(plan->off.p + nrays, &total, sizeof(total), hipMemcpyHostToDevice, st));
        if (plan->sorted) { // the order the key kernel and the sort of this call made, and its keys for the read-out
            HIPCHK(c, plan->order.reserve(nrays)); HIPCHK(c, plan->keys.reserve(nrays));
            HIPCHK(c, hipMemcpyAsync(plan->order.p, c->rs_order.p, nrays * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(plan->keys.p, c->rs_keys.p, nrays * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
            plan->spheres = c->rs_last_spheres;
        }
        unsigned long long missed = 0;
        if (total) {
            a.pl_len = plan->len.p; a.pl_off = plan->off.p; a.pl_fill = plan->list.p; a.pl_words = words.p;
            a.queue = plan->long_ids.p; a.queue_cap = (uint32_t)plan->long_rays; // the short kernel files the long rays into the plan's queue
            launch_ray_plan_fill(a, b.grid, b.src, st);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&missed, words.p + RAY_PLAN_MISMATCH, sizeof(missed), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(c, hipStreamSynchronize(st)); // complete: usable on any stream
        if (missed) return fail(c, VRT_HIP_ERR_HIP, "ray_plan_create: " + std::to_string(missed) + " rays missed the list length the count pass found");
    }
    plan->scene_n = c->n; plan->cull_gen = c->cull_gen;
    c->plans.push_back(plan.get());
    *out = plan.release();
    return VRT_HIP_OK;
}

int vrt_hip_ray_plan_create(vrt_hip_ctx *c, size_t nrays, const float *origins, int origin_per_ray, const float *dirs, vrt_hip_ray_plan **out)
{
    if (!c || !out) return VRT_HIP_ERR_INVALID;
    *out = nullptr;
    if (nrays && (!origins || !dirs)) return fail(c, VRT_HIP_ERR_INVALID, "ray_plan_create: NULL origins or directions");
    if (nrays > 0xFFFFFFF0ull) return fail(c, VRT_HIP_ERR_INVALID, "ray_plan_create: more than 2^32 - 16 rays in one plan");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // an earlier bundle may still read the staging buffers
    if (nrays) {
        const size_t no = (origin_per_ray ? nrays : 1) * 3;
        HIPCHK(c, c->rays_in[0].reserve(no)); HIPCHK(c, c->rays_in[1].reserve(nrays * 3));
        HIPCHK(c, hipMemcpyAsync(c->rays_in[0].p, origins, no * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->rays_in[1].p, dirs, nrays * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    return vrt_hip_ray_plan_create_device(c, nrays, c->rays_in[0].p, origin_per_ray, c->rays_in[1].p, c->stream, out);
}

int vrt_hip_ray_plan_destroy(vrt_hip_ctx *c, vrt_hip_ray_plan *plan)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!plan) return VRT_HIP_OK;
    if (!plan_of(c, plan)) return fail(c, VRT_HIP_ERR_INVALID, "ray_plan_destroy: not a plan of this context");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // bundles in flight read its lists
    if (c->plan == plan) { c->plan = nullptr; c->plan_flags = 0; }
    if (c->rs_last_plan == plan) { c->rs_last_plan = nullptr; c->rs_last_valid = false; }
    c->plans.erase(std::find(c->plans.begin(), c->plans.end(), plan));
    delete plan;
    return VRT_HIP_OK;
}

int vrt_hip_set_ray_plan(vrt_hip_ctx *c, vrt_hip_ray_plan *plan, int flags)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (plan && !plan_of(c, plan)) return fail(c, VRT_HIP_ERR_INVALID, "set_ray_plan: not a plan of this context");
    if (flags != 0 && flags != VRT_HIP_PLAN_KEEP_LISTS) return fail(c, VRT_HIP_ERR_INVALID, "set_ray_plan: flags is neither 0 nor VRT_HIP_PLAN_KEEP_LISTS");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = quiesce(c); if (rc) return rc; } // bundles in flight keep the lists they were enqueued with
    c->plan = plan; c->plan_flags = plan ? flags : 0;
    return VRT_HIP_OK;
}

int vrt_hip_get_ray_plan_info(vrt_hip_ctx *c, vrt_hip_ray_plan *plan, vrt_hip_ray_plan_info *out)
{
    if (!c || !out) return VRT_HIP_ERR_INVALID;
    *out = vrt_hip_ray_plan_info{};
    if (!plan_of(c, plan)) return fail(c, VRT_HIP_ERR_INVALID, "get_ray_plan_info: not a plan of this context");
    out->rays = plan->nrays; out->entries = plan->entries; out->short_rays = plan->nrays - plan->long_rays; out->long_rays = plan->long_rays;
    out->longest = plan->longest; out->scratch_rays = plan->scratch_rays; out->bytes = plan->bytes();
    out->sorted = plan->sorted; out->indexed = plan->indexed; out->scene_n = plan->scene_n; out->cull_generation = plan->cull_gen;
    return VRT_HIP_OK;
}

int vrt_hip_get_ray_plan_lists(vrt_hip_ctx *c, vrt_hip_ray_plan *plan, uint64_t *offsets, uint32_t *entries)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!plan_of(c, plan)) return fail(c, VRT_HIP_ERR_INVALID, "get_ray_plan_lists: not a plan of this context");
    if (!offsets) return fail(c, VRT_HIP_ERR_INVALID, "get_ray_plan_lists: NULL offsets");
    HIPCHK(c, hipSetDevice(c->device));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the offsets are copied as they stand");
    if (!plan->nrays) { offsets[0] = 0; return VRT_HIP_OK; }
    HIPCHK(c, hipMemcpy(offsets, plan->off.p, (plan->nrays + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (entries && plan->entries) HIPCHK(c, hipMemcpy(entries, plan->list.p, (size_t)plan->entries * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VRT_HIP_OK;
}

int vrt_hip_get_ray_index_perm(vrt_hip_ctx *c, uint32_t *out, size_t cap)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = rebuild_tables(c); if (rc) return rc; }
    if (!c->ray_index || c->ray_index_dirty) return fail(c, VRT_HIP_ERR_INVALID, "get_ray_index_perm: the index is off or not built yet");
    if (c->n && (!out || cap < c->n)) return fail(c, VRT_HIP_ERR_INVALID, "get_ray_index_perm: buffer too small");
    { int rc = quiesce(c); if (rc) return rc; } // waits for the build
    if (c->n) HIPCHK(c, hipMemcpy(out, c->ri_perm.p, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VRT_HIP_OK;
}

} // extern "C"
