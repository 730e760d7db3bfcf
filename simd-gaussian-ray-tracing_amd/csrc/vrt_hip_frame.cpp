// vrt_hip_frame.cpp -- the frame pipeline of libvrt_hip.so: one frame's host work (plan_frame), its launches (issue_frame), the
// frame entry points of the C ABI and frame batches.  There is no CPU fallback anywhere in this file.
//
// A frame on its stream (the caller's, for the *_device entry points):
//   build_tile_lists_kernel  the list kernel, only when tiles / rays / origin / options changed: the reference's tile sets (rt.cpp:29-69,
//                            or the caller's lists) intersected with a tile-level cull, and the cells' lists and queues where a tile's
//                            cells fit one workgroup (otherwise build_cell_lists_kernel behind it).  It carries the per-origin table
//                            (oc = mu - origin, |oc|^2; prep_frame_kernel only when no list kernel runs) and files the tile cones of a new camera
//   render_kernel            the block kernel: one wavefront per 8x8 pixel block of the cells with short lists
//   order_dense_kernel       the dense queue, longest list first; only when dense work is expected
//   render_table_kernel      the whole dense queue (a block it declines it shades exactly itself) -- or, with table mode off,
//                            render_dense_kernel, the exact dense kernel; left out when a frame of this state reported no dense work
// A batch: the *_batch variants of the same kernels with the frame as grid.y, and one set-up launch for the per-origin tables and
// the cone tables of the frames that need new ones.
#include <algorithm>
#include <cstring>
#include <string>

#include "vrt_hip_ctx.hpp"

using namespace vrtk;

BinArgs bin_args(const vrt_hip_ctx *c)
{
    BinArgs a{};
    a.mu_sig = c->mu_sig.p; a.gA = c->gA.p; a.gB = c->gB.p; a.n = c->n;
    // the chunk test costs a round trip of its own (the rows can only be asked for after it): worth it where the per-Gaussian pass is long
    a.chunks = (c->tune.use_chunks == 2 || (c->tune.use_chunks == 1 && c->n > 8192u)) ? c->gChunk.p : nullptr;
    for (int i = 0; i < 16; ++i) a.V.m[i] = c->view[i];
    a.xc = c->xc.p; a.yc = c->yc.p; a.tw = c->tw; a.th = c->th; a.tiles_w = c->tiles_w;
    return a;
}

namespace {

RayGen ray_gen(const vrt_hip_ctx *c, const float origin[3])
{
    RayGen r;
    r.xs = c->plane_mode ? c->xs.p : nullptr; r.ys = c->plane_mode ? c->ys.p : nullptr;
    r.zs = c->plane_mode ? c->zs.p : nullptr;
    for (int i = 0; i < 3; ++i) {
        r.origin[i] = origin[i]; r.pos[i] = c->cam_pos[i]; r.right[i] = c->cam_right[i]; r.up[i] = c->cam_up[i];
        r.front[i] = c->cam_front[i];
    }
    r.focal = c->focal;
    r.inv_half_w = 1.f / (c->w / 2.f); r.inv_half_h = 1.f / (c->h / 2.f);
    r.width = c->w; r.height = c->h;
    r.view_mode = (c->view_mode && !c->plane_mode) ? 1 : 0;
    for (int i = 0; i < 3; ++i) { r.m0[i] = c->inv_view[i]; r.m1[i] = c->inv_view[4 + i]; r.m3[i] = c->inv_view[12 + i]; }
    r.half_w = c->w / 2.f; r.half_h = c->h / 2.f;
    return r;
}

enum OutMode { OUT_RASTER = 0, OUT_COMPACT = 1, OUT_SPARSE = 2 };

// One frame, planned: what its kernels take (a FrameArgs, filled where the caller keeps it: a local, or a row of a batch's pinned
// ring) and these launch facts.  plan_frame() makes both and hands them to its caller; nothing of them stays on the context.
// kept: no list kernel (the last frame's lists, or a rank without tiles); fused: one kernel; or the tile kernel + the one-wave-per-cell
// kernel; or the cell kernel alone over the caller's lists as they are (no tile-level cull possible)
enum ListPath { LISTS_KEPT, LISTS_FUSED, LISTS_TILE_AND_CELL, LISTS_CELL_ONLY };
enum PrepTable { PREP_THERE, PREP_IN_LIST_KERNEL /* BinArgs::prep_gA */, PREP_OWN_LAUNCH /* launch_prep_frame */ }; // the per-origin table (gA)
struct FramePlan {
    ListPath lists;
    bool from_list, chunks;  // the tile kernel reads caller-made lists; it tests chunks first
    uint32_t list_grid, render_grid, dense_grid;
    PrepTable prep;
    bool cones_new;          // no row of the cone table carries this camera's tag: the list kernel files them (a batch: its cone launch)
    bool order, no_dense, table; // the dense queue is sorted; the dense launch is left out; table kernel or exact dense kernel
};

TileLists work_lists(const vrt_hip_ctx *c)
{
    TileLists t = tile_geometry(c);
    t.cull_ref_n = c->tune.cull_ref_n;
    t.floor_x = exp_floor_x(c->exp_kind);
    if (c->tile_mode == TILES_DEVICE) {
        t.start = c->w_start.p; t.count = c->w_count.p; t.indices = c->w_indices.p;
    } else if (c->work_is_ref) {
        t.start = c->ref_start.p; t.count = c->ref_count.p;
        t.indices = c->tile_mode == TILES_NONE ? c->iota.p : c->ref_indices.p;
    } else {
        t.start = c->ref_start.p; t.count = c->w_count.p; t.indices = c->w_indices.p;
    }
    return t;
}

// Queue counters come in two sets used by alternate list generations: a fused list kernel ADDS to its set
// (cleared one generation earlier by its predecessor) and clears the other set for its successor -- no memset
// node on the per-frame path.
CellGrid cell_grid(const vrt_hip_ctx *c)
{
    CellGrid g{};
    uint32_t *cnt = c->c_counters.p + 8 * (c->list_gen & 1);
    g.cells_x = c->cells_x; g.cells_y = c->cells_y; g.cstride = c->cstride;
    g.count = c->c_count.p; g.indices = c->c_indices.p; g.active = c->c_active.p; g.n_cells = c->n_cells;
    g.dense = c->c_dense.p; g.dense_sorted = c->c_dense_sorted.p; g.scratch = c->c_scratch.p; g.slot = c->c_slot.p;
    g.n_active = cnt; g.n_dense = cnt + 2;
    g.n_light = cnt + 1; g.light_threshold = c->lists_light; // as the lists in the buffers were built
    g.dense_next = cnt + 3;
    g.overflow = c->c_overflow.p; g.n_overflow = cnt + 4;
    g.table_hx = table_on(c) ? c->table_hx : 0.f; g.table_budget = c->table_budget; g.table_adapt = c->tune.table_adapt; g.table_room = c->tune.table_room;
    g.claim_early = c->tune.claim_early;
    // prune_list sums sigma*mag*exp(-x) in units of the TILE level's eps (cull_x = ln(sigma*mag / eps_eff), rebuild_tables)
    g.prune_budget = (c->cull_eps > 0.f) ? c->cull_prune * (c->tune.cull_ref_n > 0.f ? c->tune.cull_ref_n : 4096.f / 3.f) * std::max(1.f, (float)c->n / 4096.f) / c->albedo_scale : 0.f;
    g.dense_threshold = 96; // longer cell lists go straight to the 16-waves-per-block kernel (must be <= PCAP)
    g.feedback = c->d_fb;
    g.dense_is_sorted = 1;
    return g;
}

// The list part of a plan: fa.bin / fuse, which list path runs and who writes the per-origin table.  fa.O is where this
// frame is rendered to; when the fused list kernel runs it clears the cells nothing can reach.
int plan_lists(vrt_hip_ctx *c, hipStream_t st, bool use_shard, FrameArgs &fa, FramePlan &p)
{
    RenderTarget &target = fa.O;
    if (!c->lists_dirty && c->lists_for_shard == (int)use_shard) {
        // a re-render from unchanged lists: only the dense kernel's work counters need a reset (no list kernel runs in such a frame)
        HIPCHK(c, hipMemsetAsync(c->c_counters.p + 8 * (c->list_gen & 1) + 3, 0, 4 * sizeof(uint32_t), st));
        return VRT_HIP_OK;
    }
    int rc = ensure_none_ref_lists(c);
    if (rc) return rc;
    const TileLists geo = tile_geometry(c);
    const size_t nt = (size_t)geo.tiles_w * geo.tiles_h;
    // the tile cone is built from corner rays: needs pinhole rays (always true for in-kernel ray generation)
    // ... and tiles that are rectangles of the image: with the reference's truncated tile size the row stride
    // tile_w*tiles_w can differ from the width (rt.h:364-365), a tile's rows then drift sideways and wrap around the
    // image edge, and its rays are no cone around its corner rays (found by tests/fuzz_parity.py: 33x100, 5 tiles)
    const bool refine = (!c->plane_mode || c->plane_affine) && geo.stride == c->w;

    // geometry of the second level and its buffers
    uint32_t n_local = (uint32_t)nt;
    const uint32_t *tile_map = nullptr;
    if (use_shard) {
        if ((rc = rebuild_shard(c))) return rc;
        n_local = c->n_local; tile_map = c->tile_map.p;
    }
    c->cells_x = (geo.tile_w + CELL - 1) / CELL; c->cells_y = (geo.tile_h + CELL - 1) / CELL;
    c->n_cells = n_local * c->cells_x * c->cells_y;
    if (c->n_cells > ACTIVE_CELL_MASK) return fail(c, VRT_HIP_ERR_INVALID, "tile grid: more than 2^24 cells of 32 x 32 pixels on one device");
    c->cstride = std::max(1u, std::min(c->n, 4096u));
    HIPCHK(c, c->c_count.reserve(c->n_cells)); HIPCHK(c, c->c_active.reserve(c->n_cells));
    HIPCHK(c, c->c_dense.reserve(c->n_cells));
    HIPCHK(c, c->c_dense_sorted.reserve(c->n_cells));
    HIPCHK(c, c->c_slot.reserve(c->n_cells));
    HIPCHK(c, c->c_scratch.reserve((size_t)c->num_cus * 4 * c->cstride)); // one slot per dense workgroup (<= 4 per CU)
    HIPCHK(c, c->c_overflow.reserve((size_t)c->n_cells * 16));
    HIPCHK(c, c->c_indices.reserve((size_t)c->n_cells * c->cstride));
    if (!c->c_counters.p) {
        HIPCHK(c, c->c_counters.reserve(16));
        HIPCHK(c, hipMemsetAsync(c->c_counters.p, 0, 16 * sizeof(uint32_t), st));
    }
    ++c->list_gen; // this build fills counter set (list_gen & 1)
    if (c->tile_mode == TILES_DEVICE && c->grid_n != c->n) { // the scene was replaced after tile_gaussians()
        HIPCHK(c, hipStreamSynchronize(st));
        if ((rc = prepare_tile_grid(c, c->tw, c->th))) return rc;
        c->last_stream = st;
    }

    BinArgs &a = fa.bin;
    a = bin_args(c);
    a.refine = refine ? 1 : 0;
    a.cull_ref_n = c->tune.cull_ref_n; a.floor_x = exp_floor_x(c->exp_kind);
    a.R = fa.R;
    a.tile_w = geo.tile_w; a.tile_h = geo.tile_h; a.stride = geo.stride;
    c->work_is_ref = false;
    if (refine) {
        std::string key((const char *)&a.R, sizeof a.R);
        const uint32_t geo_key[6] = { geo.tile_w, geo.tile_h, geo.stride, geo.tiles_w, geo.tiles_h, c->plane_gen };
        key.append((const char *)geo_key, sizeof geo_key);
        a.tiles_w = geo.tiles_w;
        // with the cells' cones when the tile's cells are filtered by the same workgroup (the fused list kernel)
        const uint32_t cpt = c->cells_x * c->cells_y;
        const uint32_t cones_cells = cpt <= (uint32_t)MAX_FUSED_CELLS ? cpt : 0u;
        const size_t rows = nt * (1 + cones_cells);
        // The table fills itself: a row is valid if it carries the tag of this camera (cone_gen); the list kernel's workgroups build the cones
        // they do not find and file them (round 3: the table's own launch cost a frame whose camera moved 5 us).  Frames of a batch get
        // theirs from one launch for the whole batch, as before (its BinArgs are the frame's bin row, its grid the cones_* of the plan).
        if (c->tile_cones.cap < 2 * rows) {
            HIPCHK(c, c->tile_cones.reserve(2 * rows));
            HIPCHK(c, hipMemsetAsync(c->tile_cones.p, 0, c->tile_cones.cap * sizeof(float4), st)); // tag 0: no camera's
            c->cone_key.clear();
        }
        if (key != c->cone_key) {
            if (++c->cone_gen == 0u) c->cone_gen = 1u;
            p.cones_new = true;
            fa.cones_tiles = a.tiles_w * geo.tiles_h;
            fa.cones_cx = cones_cells ? c->cells_x : 0u; fa.cones_cy = cones_cells ? c->cells_y : 0u;
            fa.cones_out = c->tile_cones.p;
            c->cone_key = key;
        }
        a.tile_cones = c->tile_cones.p; a.cones_cells = cones_cells; a.cone_gen = c->cone_gen; a.cones_known = p.cones_new ? 0 : 1;
    }
    const bool device_bin = c->tile_mode == TILES_DEVICE;
    // one fused kernel when a tile's cells fit one workgroup's waves; otherwise tile kernel + one-wave-per-cell kernel
    const bool fuse = c->cells_x * c->cells_y <= (uint32_t)MAX_FUSED_CELLS && (device_bin || refine);
    c->lists_light = (fuse && !target.sparse) ? c->light_cells : 0u;
    FuseArgs &f = fa.fuse;
    f.enabled = fuse ? 1 : 0;
    f.tile_map = fuse ? tile_map : nullptr;
    f.C = cell_grid(c);
    if (fuse) { f.O = target; f.do_clear = target.sparse ? 0 : 1; }
    c->timeline_tiles = 0;
    if (fuse && c->tune.timeline) {
        c->timeline_tiles = n_local;
        HIPCHK(c, c->d_timeline_lists.reserve((size_t)n_local * 8));
        HIPCHK(c, hipMemsetAsync(c->d_timeline_lists.p, 0, (size_t)n_local * 8 * sizeof(unsigned long long), st));
        f.timeline = c->d_timeline_lists.p;
    }
    a.zero8 = fuse ? nullptr : c->c_counters.p + 8 * (c->list_gen & 1);
    if (device_bin) {
        a.out_start = c->w_start.p; a.out_indices = c->w_indices.p; a.out_count = c->w_count.p;
    } else if (refine) {
        const size_t total = c->tile_mode == TILES_NONE ? c->n : c->ref_indices.cap;
        HIPCHK(c, c->w_count.reserve(nt)); HIPCHK(c, c->w_indices.reserve(total));
        a.in_start = c->ref_start.p; a.in_count = c->ref_count.p;
        a.in_indices = c->tile_mode == TILES_NONE ? c->iota.p : c->ref_indices.p;
        a.out_start = c->ref_start.p; a.out_indices = c->w_indices.p; a.out_count = c->w_count.p;
    } else {
        c->work_is_ref = true;
    }
    if (fuse) {
        a.next_zero8 = c->c_counters.p + 8 * ((c->list_gen + 1) & 1); // cleared for the next generation by workgroup 0
        if (n_local) {
            p.lists = LISTS_FUSED; p.list_grid = n_local;
        } else {
            // a rank that owns no tile (more ranks than tiles) launches no list kernel: nobody adds to this generation's
            // counters and nobody clears the next one's -- do both here, or the next render would add to stale counts
            // (found by tests/fuzz_parity.py: 4 tiles on 5 and 8 ranks)
            HIPCHK(c, hipMemsetAsync(c->c_counters.p, 0, 16 * sizeof(uint32_t), st));
        }
        target.cleared = 1;
    } else {
        p.lists = c->work_is_ref ? LISTS_CELL_ONLY : LISTS_TILE_AND_CELL; p.list_grid = (uint32_t)nt;
        if (c->work_is_ref) HIPCHK(c, hipMemsetAsync(a.zero8, 0, 8 * sizeof(uint32_t), st)); // no tile kernel clears this generation's counters
        if (target.sparse) target.cleared = 1; // a sparse shard stores no empty cells: nothing to clear
    }
    p.from_list = !device_bin; p.chunks = device_bin && a.chunks && a.refine;
    // a.R.origin is the origin the table is for; the cell kernel reads the table: if no tile kernel writes it, it gets its own launch
    if (p.prep == PREP_OWN_LAUNCH && p.lists != LISTS_CELL_ONLY && p.lists != LISTS_KEPT) p.prep = PREP_IN_LIST_KERNEL;
    c->lists_dirty = false;
    c->lists_for_shard = (int)use_shard;
    return VRT_HIP_OK;
}

// CellGrid::claim_early for a block-kernel launch of `grid` waves per frame: the variant that claims its next queue entry early, for
// frames with (by an earlier frame's report, however old: speed only) at least grid / claim_early more blocks than the grid has waves
int claim_early_for(const vrt_hip_ctx *c, uint32_t grid)
{
    const uint32_t seen_blocks = (c->h_fb.p && !c->stats_on) ? c->h_fb.p[1] : 0u;
    const bool many = c->tune.claim_early > 0 && seen_blocks > grid && (uint64_t)(seen_blocks - grid) * (uint32_t)c->tune.claim_early >= grid;
    return many ? c->tune.claim_early : 0;
}

// Retained frame buffer (vrt_hip_frame's own buffer; vrt_hip_frame_retained_device for a caller's): `o.image` still holds this
// context's previous frame at this geometry, so the list kernel clears only the cells that went dark (RenderTarget::stamp).
// One history per context, for ONE buffer: another buffer, image size, tile grid or background starts a new one with a
// full clear.  Comes after the plan's hand-over from the last stream: the previous frame's list and block kernels may still be
// writing the stamps and the image that the memsets below reset on THIS stream.
int retained_begin(vrt_hip_ctx *c, const TileLists &geo, RenderTarget &o, hipStream_t st)
{
    const size_t cells = (size_t)geo.tiles_w * geo.tiles_h * ((geo.tile_w + CELL - 1) / CELL) * ((geo.tile_h + CELL - 1) / CELL);
    vrt_hip_ctx::OwnGeometry sig;
    sig.w = c->w; sig.h = c->h; sig.tiles_w = geo.tiles_w; sig.tiles_h = geo.tiles_h; sig.tile_w = geo.tile_w; sig.tile_h = geo.tile_h;
    sig.background = (o.pack_flags & VRT_ALPHA_COMPUTED) ? 0u : 0xFF000000u; sig.image = o.image;
    if (!(c->tune.retain_frame && cells > 0 && cells < (1u << 28) && c->world == 1)) { c->own_seq = 0; return VRT_HIP_OK; }
    if (!(sig == c->own_sig) || c->own_seq == 0 || c->own_seq >= 0xFFFFFFF0u || c->own_stamp.cap < cells) {
        if (c->own_stamp.cap < cells) { int rc = quiesce(c); if (rc) return rc; c->last_stream = st; } // frames in flight write the old stamp buffer
        HIPCHK(c, c->own_stamp.reserve(cells));
        HIPCHK(c, hipMemsetAsync(c->own_stamp.p, 0, cells * sizeof(uint32_t), st));
        if (!(sig == c->own_sig)) HIPCHK(c, hipMemsetAsync(o.image, 0, (size_t)c->w * c->h * 4, st)); // pixels no tile of the NEW grid covers read 0
        c->own_sig = sig;
        c->own_seq = 1; // stamps of 0 = "never lit": with seq 1 every empty cell compares against 0 = seq - 1 and is cleared
    } else {
        ++c->own_seq;
    }
    o.stamp = c->own_stamp.p; o.stamp_seq = c->own_seq;
    return VRT_HIP_OK;
}

// One frame's host work: checks, rebuilds, reserves, first-use memsets, generations.  Launches no kernel; the memsets it
// enqueues on `st` clear what neither a list kernel nor prep_frame_kernel (gA only) reads or writes, so they precede those launches.
// `retain`: d_image holds this context's previous frame (retained_begin).  `t0`: a timed frame's first event ("before lists"), recorded
// behind the hand-over and ahead of everything the frame enqueues; null otherwise.
int plan_frame(vrt_hip_ctx *c, const float origin[3], int pack_flags, uint32_t *d_image, float4 *d_rad, hipStream_t st, int out_mode,
               bool retain, hipEvent_t t0, FrameArgs &fa, FramePlan &p)
{
    fa = FrameArgs{};
    p = FramePlan{};
    int rc = check_ready(c);
    if (rc) return rc;
    const TileLists geo = tile_geometry(c);
    if (geo.tile_w == 0 || geo.tile_h == 0) return fail(c, VRT_HIP_ERR_INVALID, "render: tile size is 0 pixels");
    const bool use_shard = c->world > 1 || out_mode != OUT_RASTER; // compact and sparse targets hold this rank's tiles only
    if ((rc = rebuild_tables(c))) return rc; // (waits for everything in flight itself, and forgets the last stream: before the hand-over)
    if ((rc = resolve_albedo_scale(c))) return rc; // the first frame of a scene set from device memory waits for one word: the prune budget needs it
    wait_for_last_stream(c, st);
    c->last_stream = st;
    if (t0) HIPCHK(c, hipEventRecord(t0, st));
    if (!c->gA_valid || memcmp(c->gA_origin, origin, 3 * sizeof(float))) {
        p.prep = PREP_OWN_LAUNCH; // unless a list kernel of this frame takes the table along (plan_lists)
        fa.prep_gA = c->gA.p; memcpy(fa.prep_origin, origin, 3 * sizeof(float));
        memcpy(c->gA_origin, origin, 3 * sizeof(float));
        c->cam_seq = c->frame_seq; // the camera moved
        c->gA_valid = true;
        c->lists_dirty = true; // the tile-level cull depends on the origin
    }
    fa.S = tables(c); fa.R = ray_gen(c, origin);
    RenderTarget &o = fa.O;
    o.image = d_image; o.radiance = d_rad; o.pack_flags = pack_flags;
    o.stats = c->stats_on ? c->d_stats.p : nullptr;
    o.compact = out_mode == OUT_COMPACT ? 1 : 0;
    if (use_shard) {
        if ((rc = rebuild_shard(c))) return rc;
        o.tile_map = c->tile_map.p; o.n_local_tiles = c->n_local;
    } else {
        o.n_local_tiles = geo.tiles_w * geo.tiles_h;
    }
    if (out_mode == OUT_SPARSE) {
        // d_image is a sparse shard buffer: header | keys | pixels of the stored cells (vrt_kernels.h, RenderTarget)
        const uint32_t sparse_cap = sparse_capacity(c);
        o.sparse = 1; o.sparse_hdr = d_image; o.keys = d_image + SPARSE_HDR_WORDS;
        o.image = d_image + sparse_pixel_offset(sparse_cap);
        o.cleared = 1;
        c->lists_dirty = true; // the list kernel files the cell keys into THIS buffer
        o.sparse_cap = sparse_cap;
    }
    if (retain && (rc = retained_begin(c, geo, o, st))) return rc;
    if ((rc = plan_lists(c, st, use_shard, fa, p))) return rc;
    if (o.stamp && !o.cleared) c->own_seq = 0; // the list kernel of this frame was not the fused one: nobody kept the stamps
    const TileLists &t = fa.T = work_lists(c);
    if (o.stats) { // the list kernels keep no statistics: these words belong to the block kernel and the dense kernels
        HIPCHK(c, hipMemsetAsync(c->d_stats.p, 0, STAT_WORDS * sizeof(unsigned long long), st));
        HIPCHK(c, hipMemsetAsync(c->d_stats.p + STAT_DENSE_T_FIRST, 0xFF, sizeof(unsigned long long), st)); // running minimum
    }
    c->timeline_items = 0;
    if (c->tune.timeline) { // the block kernel's stamps; the list kernel's go to a buffer of their own (d_timeline_lists)
        c->timeline_items = (size_t)c->n_cells * 16;
        HIPCHK(c, c->d_timeline.reserve(c->timeline_items * 5));
        HIPCHK(c, hipMemsetAsync(c->d_timeline.p, 0, c->timeline_items * 5 * sizeof(unsigned long long), st));
        o.timeline = c->d_timeline.p;
    }
    const uint32_t bx = (t.tile_w + BLOCK_W - 1) / BLOCK_W, by = (t.tile_h + BLOCK_H - 1) / BLOCK_H;
    c->last.blocks = (uint64_t)o.n_local_tiles * bx * by;
    c->last.rays = (uint64_t)o.n_local_tiles * t.tile_w * t.tile_h;
    // persistent grid: 12 one-wave workgroups per CU (three per SIMD at 145 VGPRs), never more than there are blocks
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)c->n_cells * 16u,
                                                       c->tune.render_grid_override ? (uint64_t)c->tune.render_grid_override
                                                                               : (uint64_t)c->num_cus * std::max(1, c->tune.render_waves_per_cu));
    if (out_mode == OUT_SPARSE && grid == 0) // a rank without cells launches no render kernel: nobody writes the header (only the block kernel does)
        HIPCHK(c, hipMemsetAsync(d_image, 0, SPARSE_HDR_WORDS * sizeof(uint32_t), st));
    // How large a dense launch?  The 16-waves-per-block kernel always runs behind the one-wave kernel (which kernel
    // shades a block depends on the block alone, so the image never depends on this heuristic); but a full launch --
    // queue sort + one 1024-thread workgroup per CU -- costs ~12 us even with empty queues.  Frames report
    // (asynchronously, CellGrid::feedback) what their dense kernel found; once a report has arrived from a frame
    // launched at least two frames after the last change of scene, rays, camera or options, and it says "nothing",
    // the launch shrinks to one workgroup and skips the sort.  A wrong guess costs speed only.
    bool expect_dense = true, camera_moved = false;
    if (c->h_fb.p && !c->stats_on && (int32_t)(c->h_fb.p[3] - c->reset_seq) >= 2) {
        expect_dense = c->h_fb.p[0] > 0 || c->h_fb.p[2] > 0;
        camera_moved = (int32_t)(c->h_fb.p[3] - c->cam_seq) < 2;
    }
    // Not a guess: which blocks are dense is a function of scene, options, rays, camera, tile grid and shard.  A report
    // from a frame that was launched AFTER the last change of any of them (sequence number above reset_seq and cam_seq)
    // and that found no dense cell and no handed-over block says the same of this frame: the dense launch -- 4.7 us of a
    // 47-us serial frame even for one idle workgroup, which also waits for 61 KB of LDS while other frames' block kernels
    // fill the CUs -- is left out.  Any change brings it back until a frame of the new state has reported.
    if (c->tune.skip_idle_dense && c->h_fb.p && !c->stats_on) {
        const uint32_t seen = c->h_fb.p[3]; // read first: what is read after it is at least as new
        p.no_dense = (int32_t)(seen - c->reset_seq) >= 1 && (int32_t)(seen - c->cam_seq) >= 1 && c->h_fb.p[0] == 0 && c->h_fb.p[2] == 0;
    }
    if (p.no_dense) ++c->last.dense_launch_skips;
    p.dense_grid = p.no_dense ? 0u : (uint32_t)std::min<uint64_t>((uint64_t)c->n_cells * 16u, (uint64_t)c->num_cus * (16 / std::min(c->tune.dense_waves, 16)));
    if (!expect_dense) p.dense_grid = std::min(p.dense_grid, (uint32_t)(camera_moved ? std::max(c->dense_idle_grid, c->num_cus / 4) : c->dense_idle_grid));
    CellGrid &cg = fa.C = cell_grid(c);
    cg.claim_early = claim_early_for(c, grid);
    cg.dense_is_sorted = expect_dense ? 1 : 0;
    cg.frame_seq = ++c->frame_seq;
    if (!c->c_rq.p) { // the work queues are the block kernel's alone
        HIPCHK(c, c->c_rq.reserve(2 * RQ_N * RQ_STRIDE));
        HIPCHK(c, hipMemsetAsync(c->c_rq.p, 0, 2 * RQ_N * RQ_STRIDE * sizeof(uint32_t), st));
    }
    if (grid) ++c->rq_gen; // a skipped launch clears nothing: the sets must not swap
    cg.rq = c->c_rq.p + (c->rq_gen & 1) * RQ_N * RQ_STRIDE;
    cg.rq_next = c->c_rq.p + ((c->rq_gen + 1) & 1) * RQ_N * RQ_STRIDE;
    p.render_grid = grid; p.order = expect_dense && !p.no_dense; p.table = table_on(c);
    return VRT_HIP_OK;
}

// What the unissued plans of a refused batch have consumed, given back: the kernels that would have kept these invariants will not run.
void abandon_plan(vrt_hip_ctx *c, hipStream_t st)
{
    // list generation: the counter set the list kernel would have cleared for the next generation is stale -- clear both, rebuild the lists
    if (c->c_counters.p && hipMemsetAsync(c->c_counters.p, 0, 16 * sizeof(uint32_t), st) != hipSuccess) (void)hipGetLastError();
    c->lists_dirty = true;
    // queue generation: likewise the work-queue set the block kernel would have cleared for the next launch
    if (c->c_rq.p && hipMemsetAsync(c->c_rq.p, 0, 2 * RQ_N * RQ_STRIDE * sizeof(uint32_t), st) != hipSuccess) (void)hipGetLastError();
    c->gA_valid = false;   // per-origin table: noted as this origin's, never written
    c->cone_key.clear();   // cone tag: handed out for this camera, no row was filed under it
}

// A planned frame's launches.  tev: a timed frame's events (0 before lists: plan_frame's t0; before render, after render, after dense), or null.
int issue_frame(vrt_hip_ctx *c, const FramePlan &p, FrameArgs &fa, hipStream_t st, hipEvent_t *tev)
{
    if (p.prep == PREP_IN_LIST_KERNEL) fa.bin.prep_gA = fa.prep_gA;
    if (p.lists == LISTS_FUSED || p.lists == LISTS_TILE_AND_CELL) launch_build_tile_lists(fa.bin, fa.fuse, p.from_list, p.list_grid, st);
    if (p.prep == PREP_OWN_LAUNCH) launch_prep_frame(fa.S, fa.prep_gA, fa.prep_origin, st); // lists unchanged, caller-made lists used as they are, a rank without tiles
    if (p.lists == LISTS_TILE_AND_CELL || p.lists == LISTS_CELL_ONLY) {
        launch_build_cell_lists(fa.S, fa.T, fa.fuse.C, fa.R, fa.O.tile_map, fa.C.n_cells, fa.bin.refine, fa.O.sparse ? fa.O.keys : nullptr, st);
        // the set the NEXT generation will add to (if it is a fused one) must be clear
        HIPCHK(c, hipMemsetAsync(c->c_counters.p + 8 * ((c->list_gen + 1) & 1), 0, 8 * sizeof(uint32_t), st));
    }
    if (tev) HIPCHK(c, hipEventRecord(tev[1], st));
    launch_render(fa.S, fa.T, fa.C, fa.R, fa.O, p.render_grid, c->exp_kind, c->erf_kind, st);
    if (tev) HIPCHK(c, hipEventRecord(tev[2], st));
    // dense queue: 16-wave workgroups pull blocks until the queue is empty (they exit at once if it is)
    if (p.order) launch_order_dense(fa.C, st);
    if (!p.no_dense) {
        // table mode (the default): the table kernel takes the whole dense queue; a block it declines it shades exactly itself
        // (dense_shade_block in its own LDS): ONE dense-path launch per frame (rounds 1-3: an exact launch behind it, idle in
        // every frame of a moving camera)
        if (p.table)
            launch_render_table(fa.S, fa.T, fa.C, fa.R, fa.O, std::min<uint32_t>(p.dense_grid, (uint32_t)c->num_cus), c->exp_kind, c->erf_kind, st);
        else
            launch_render_dense(fa.S, fa.T, fa.C, fa.R, fa.O, p.dense_grid, c->tune.dense_waves, c->exp_kind, c->erf_kind, st);
    }
    if (tev) {
        if (c->timing_full) HIPCHK(c, hipEventRecord(tev[3], st));
        ++c->timing_count;
    }
    HIPCHK(c, hipGetLastError());
    return VRT_HIP_OK;
}

// A single frame: planned, then issued.
int render_frame(vrt_hip_ctx *c, const float origin[3], int pack_flags, uint32_t *d_image, float4 *d_rad, hipStream_t st, int out_mode, bool retain)
{
    int rc;
    hipEvent_t *tev = nullptr;
    if (c->timing_on && (c->timing_frame++ % c->timing_period) == 0) {
        if ((rc = ensure_timing_ring(c))) return rc;
        tev = &c->tev[4 * (c->timing_count % vrt_hip_ctx::TIMING_RING)];
    }
    FrameArgs fa;
    FramePlan p;
    if ((rc = plan_frame(c, origin, pack_flags, d_image, d_rad, st, out_mode, retain, tev && c->timing_full ? tev[0] : nullptr, fa, p))) return rc;
    return issue_frame(c, p, fa, st, tev);
}

} // namespace

int frame_own_image(vrt_hip_ctx *c, float tw, float th, const float view[16], const float origin[3], int pack_flags)
{
    int rc = check_ready(c);
    if (rc) return rc;
    const size_t npix = (size_t)c->w * c->h;
    if (c->d_image.cap < npix) { // first frame at this size: pixels no tile covers read 0
        HIPCHK(c, c->d_image.reserve(npix));
        HIPCHK(c, hipMemsetAsync(c->d_image.p, 0, npix * 4, c->stream));
        c->own_seq = 0;
    }
    // Retained frame buffer: d_image is written by nothing but this function and vrt_hip_render (which ends the history), so
    // an empty cell that was empty in the previous frame already holds the background.
    return vrt_hip_frame_retained_device(c, tw, th, view, origin, pack_flags, c->d_image.p, c->stream);
}

extern "C" {

int vrt_hip_render_device(vrt_hip_ctx *c, const float origin[3], int pack_flags, uint32_t *d_image, float *d_radiance, void *hip_stream)
{
    if (!c || !origin) return VRT_HIP_ERR_INVALID;
    return render_frame(c, origin, pack_flags, d_image, (float4 *)d_radiance, (hipStream_t)hip_stream, OUT_RASTER, false);
}

int vrt_hip_frame_device(vrt_hip_ctx *c, float tw, float th, const float view[16], const float origin[3], int pack_flags,
                         uint32_t *d_out, int shard, void *hip_stream)
{
    if (!c || !origin || !d_out) return VRT_HIP_ERR_INVALID;
    int rc = vrt_hip_tile_gaussians_device(c, tw, th, view, hip_stream);
    return rc ? rc : render_frame(c, origin, pack_flags, d_out, nullptr, (hipStream_t)hip_stream, shard ? OUT_COMPACT : OUT_RASTER, false);
}

int vrt_hip_frame_retained_device(vrt_hip_ctx *c, float tw, float th, const float view[16], const float origin[3], int pack_flags,
                                  uint32_t *d_out, void *hip_stream)
{
    if (!c || !origin || !d_out) return VRT_HIP_ERR_INVALID;
    int rc = vrt_hip_tile_gaussians_device(c, tw, th, view, hip_stream);
    if (!rc) rc = render_frame(c, origin, pack_flags, d_out, nullptr, (hipStream_t)hip_stream, OUT_RASTER, true);
    if (rc) c->own_seq = 0;
    return rc;
}

int vrt_hip_frame(vrt_hip_ctx *c, float tw, float th, const float view[16], const float origin[3], int pack_flags,
                  uint32_t *image_out, int wait)
{
    if (!c || !origin || !view) return VRT_HIP_ERR_INVALID;
    int rc = frame_own_image(c, tw, th, view, origin, pack_flags);
    if (rc) return rc;
    const size_t npix = (size_t)c->w * c->h;
    if (image_out) HIPCHK(c, hipMemcpyAsync(image_out, c->d_image.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (image_out || wait) HIPCHK(c, hipStreamSynchronize(c->stream));
    return VRT_HIP_OK;
}

int vrt_hip_render(vrt_hip_ctx *c, const float origin[3], int pack_flags, uint32_t *image_out, float *radiance_out)
{
    if (!c || !origin) return VRT_HIP_ERR_INVALID;
    int rc = check_ready(c);
    if (rc) return rc;
    const size_t npix = (size_t)c->w * c->h;
    HIPCHK(c, c->d_image.reserve(npix));
    c->own_seq = 0; // the library's frame buffer gets another image: vrt_hip_frame's retained history of it ends
    if (radiance_out) HIPCHK(c, c->d_rad.reserve(npix));
    HIPCHK(c, hipMemsetAsync(c->d_image.p, 0, npix * 4, c->stream));
    if (radiance_out) HIPCHK(c, hipMemsetAsync(c->d_rad.p, 0, npix * 16, c->stream));
    // the static tables outside the timed window (list building is part of a frame, like the reference's tiling)
    if ((rc = rebuild_tables(c))) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    rc = render_frame(c, origin, pack_flags, c->d_image.p, radiance_out ? c->d_rad.p : nullptr, c->stream, OUT_RASTER, false);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last.kernel_ms = ms;
    if (c->stats_on && (rc = read_stats(c))) return rc;
    if (c->timeline_items) print_timeline(c);
    if (image_out) HIPCHK(c, hipMemcpy(image_out, c->d_image.p, npix * 4, hipMemcpyDeviceToHost));
    if (radiance_out) HIPCHK(c, hipMemcpy(radiance_out, c->d_rad.p, npix * 16, hipMemcpyDeviceToHost));
    return VRT_HIP_OK;
}

int vrt_hip_render_shard_device(vrt_hip_ctx *c, const float origin[3], int pack_flags, uint32_t *d_shard, void *hip_stream)
{
    if (!c || !origin || !d_shard) return VRT_HIP_ERR_INVALID;
    return render_frame(c, origin, pack_flags, d_shard, nullptr, (hipStream_t)hip_stream, OUT_COMPACT, false);
}

int vrt_hip_frame_sparse_device(vrt_hip_ctx *c, float tw, float th, const float view[16], const float origin[3], int pack_flags,
                                uint32_t *d_sparse, void *hip_stream)
{
    if (!c || !origin || !d_sparse) return VRT_HIP_ERR_INVALID;
    if ((uintptr_t)d_sparse % 16) return fail(c, VRT_HIP_ERR_INVALID, "frame_sparse: the shard buffer must be 16-byte aligned");
    int rc = vrt_hip_tile_gaussians_device(c, tw, th, view, hip_stream);
    return rc ? rc : render_frame(c, origin, pack_flags, d_sparse, nullptr, (hipStream_t)hip_stream, OUT_SPARSE, false);
}

int vrt_hip_frame_batch_device(vrt_hip_ctx *const *ctxs, int n, float tw, float th, const float *views, const float *origins,
                               int pack_flags, uint32_t *const *d_out, int out_kind, void *hip_stream)
{
    if (!ctxs || n < 1 || !ctxs[0]) return VRT_HIP_ERR_INVALID;
    vrt_hip_ctx *c0 = ctxs[0];
    if (!views || !origins || !d_out) return fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: null argument");
    if (n > 64) return fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: at most 64 frames per batch");
    if (out_kind < OUT_RASTER || out_kind > OUT_SPARSE) return fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: out_kind is 0 (frame), 1 (compact shard) or 2 (sparse shard)");
    hipStream_t st = (hipStream_t)hip_stream;
    for (int i = 0; i < n; ++i) {
        vrt_hip_ctx *c = ctxs[i];
        if (!c || !d_out[i]) return fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: null context or output");
        for (int k = 0; k < i; ++k)
            if (ctxs[k] == c) return fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: a context holds ONE frame's lists and queues -- every frame of a batch needs its own");
        if (c->device != c0->device || c->exp_kind != c0->exp_kind || c->erf_kind != c0->erf_kind || c->tune.dense_waves != c0->tune.dense_waves ||
            c->table_hx != c0->table_hx || c->table_budget != c0->table_budget || c->cull_prune != c0->cull_prune || c->cull_eps != c0->cull_eps)
            return fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: the contexts differ in device or in Exp / Erf / dense-kernel / table options");
        if (c->w != c0->w || c->h != c0->h || c->n != c0->n || c->rank != c0->rank || c->world != c0->world)
            return fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: the frames differ in image size, scene size or shard");
        if (out_kind == OUT_SPARSE && (uintptr_t)d_out[i] % 16) return fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: sparse shard buffers must be 16-byte aligned");
    }
    HIPCHK(c0, hipSetDevice(c0->device));
    // argument rows: slot (batch_seq % BATCH_SLOTS) of the pinned ring, copied to the same slot of the device ring
    if ((size_t)n > c0->batch_cap) {
        int rc = quiesce(c0);
        if (rc) return rc;
        HIPCHK(c0, hipStreamSynchronize(st));
        c0->batch_cap = 0;
        const size_t cap = std::max<size_t>(16, (size_t)n);
        HIPCHK(c0, c0->batch_host.alloc(cap * vrt_hip_ctx::BATCH_SLOTS, hipHostMallocDefault));
        HIPCHK(c0, c0->batch_dev.reserve(cap * vrt_hip_ctx::BATCH_SLOTS));
        c0->batch_cap = cap;
        for (auto &e : c0->batch_copied) if (!e) HIPCHK(c0, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const uint32_t slot = c0->batch_seq++ % vrt_hip_ctx::BATCH_SLOTS;
    if (c0->batch_seq > (uint32_t)vrt_hip_ctx::BATCH_SLOTS) HIPCHK(c0, hipEventSynchronize(c0->batch_copied[slot])); // the copy that last read this slot
    FrameArgs *rows = c0->batch_host.p + (size_t)slot * c0->batch_cap;
    FrameArgs *d_rows = c0->batch_dev.p + (size_t)slot * c0->batch_cap;

    // every frame's host work and memsets as for a single frame; its plan becomes a row, its launch facts must be the first frame's
    FramePlan p, p0{};
    int failed = VRT_HIP_OK, touched = 0;
    uint32_t dgrid = 0;
    while (touched < n && !failed) {
        const int i = touched++;
        vrt_hip_ctx *c = ctxs[i];
        int rc = vrt_hip_tile_gaussians_device(c, tw, th, views + 16 * (size_t)i, hip_stream);
        if (!rc) rc = plan_frame(c, origins + 3 * (size_t)i, pack_flags, d_out[i], nullptr, st, out_kind, false, nullptr, rows[i], p);
        if (!rc && (p.lists == LISTS_TILE_AND_CELL || p.lists == LISTS_CELL_ONLY))
            rc = fail(c, VRT_HIP_ERR_INVALID, "frame batch: tiles of more than 64 cells (or rays that are no pinhole bundle) "
                                              "need the two-kernel list path, which is not batched");
        if (rc) {
            failed = c == c0 ? rc : fail(c0, rc, std::string("frame_batch: frame ") + std::to_string(i) + ": " + c->err);
            break;
        }
        if (i == 0) p0 = p;
        if (p.lists != p0.lists || p.from_list != p0.from_list || p.list_grid != p0.list_grid || p.render_grid != p0.render_grid)
            failed = fail(c0, VRT_HIP_ERR_INVALID, "frame_batch: the frames differ in image size, tile grid, shard or scene size");
        // the set-up kernels of the batch: one prep launch and one cone launch for all frames (launch_frame_setup_batch), one queue sort
        FrameArgs &row = rows[i];
        row.do_prep = p.prep != PREP_THERE; row.do_order = p.order;
        if (p.cones_new) { row.do_cones = 1; row.bin.cones_known = 1; }
        dgrid = std::max(dgrid, p.dense_grid);
    }
    if (failed) { // no frame of the batch is issued
        for (int i = 0; i < touched; ++i) abandon_plan(ctxs[i], st);
        return failed;
    }
    // one-wave kernel: the persistent grid of ONE frame fills the GPU; n frames share it -- so a frame of a batch has 1/n of the waves and
    // that many more queue entries: the variant that claims them early is chosen against the per-frame grid
    const uint32_t full_grid = p0.render_grid;
    const uint32_t rgrid = full_grid ? std::min(full_grid, std::max(1u, (full_grid + (uint32_t)n - 1) / (uint32_t)n)) : 0u;
    bool claim = false;
    for (int i = 0; i < n; ++i) claim |= (rows[i].C.claim_early = claim_early_for(ctxs[i], rgrid)) != 0;
    HIPCHK(c0, hipMemcpyAsync(d_rows, rows, (size_t)n * sizeof(FrameArgs), hipMemcpyHostToDevice, st));
    HIPCHK(c0, hipEventRecord(c0->batch_copied[slot], st));
    launch_frame_setup_batch(d_rows, rows, (uint32_t)n, st); // per-origin tables and cone tables of the frames that need new ones
    if (p0.lists == LISTS_FUSED) // (same scene size and geometry in every frame: checked above)
        launch_build_tile_lists_batch(d_rows, (uint32_t)n, p0.from_list, p0.chunks, p0.list_grid, st);
    launch_render_batch(d_rows, (uint32_t)n, rgrid, claim, c0->exp_kind, c0->erf_kind, st);
    launch_order_dense_batch(d_rows, rows, (uint32_t)n, st);
    if (p0.table)
        launch_render_table_batch(d_rows, (uint32_t)n, std::min<uint32_t>(dgrid, (uint32_t)c0->num_cus), (uint64_t)rows[0].R.width * rows[0].R.height,
                                  c0->exp_kind, c0->erf_kind, st);
    else
        launch_render_dense_batch(d_rows, (uint32_t)n, dgrid, c0->tune.dense_waves, c0->exp_kind, c0->erf_kind, st);
    HIPCHK(c0, hipGetLastError());
    return VRT_HIP_OK;
}

} // extern "C"
