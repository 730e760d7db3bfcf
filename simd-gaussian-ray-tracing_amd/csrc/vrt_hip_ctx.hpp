// vrt_hip_ctx.hpp -- internal to libvrt_hip.so: the context behind the C ABI (include/vrt_hip.h), the owning buffer types and
// what the host runtime's translation units share (vrt_hip_api.cpp: context, setters, tiles, shard map, tables;
// vrt_hip_frame.cpp: frame pipeline; vrt_hip_assembly.cpp: shard assembly; vrt_hip_query.cpp: point queries; vrt_hip_rays.cpp: ray and transmittance bundles; vrt_hip_diag.cpp: stats, kernel timing, timelines).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/vrt_hip.h"
#include "vrt_kernels.h"

#pragma GCC visibility push(hidden) // nothing declared here is part of the library's ABI

// Device memory owned by its holder: freed when the holder goes (hipFree waits for the device first).  reserve() grows
// without keeping the contents; release() frees now.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); std::swap(p, o.p); std::swap(cap, o.cap); }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void **)&p, (n ? n : 1) * sizeof(T));
        if (e == hipSuccess) cap = n ? n : 1;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Pinned host memory owned by its holder.
template <typename T>
struct PinnedBuf {
    T *p = nullptr;
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p, o.p); return *this; }
    ~PinnedBuf() { if (p) (void)hipHostFree((void *)p); }
    hipError_t alloc(size_t n, unsigned flags) { *this = PinnedBuf{}; return hipHostMalloc((void **)&p, n * sizeof(T), flags); }
};

// Every VRT_HIP_* setting of the host runtime, read from the environment once, by vrt_hip_create (read_tuning).  The
// initialisers are the defaults.
struct Tuning {
    int render_waves_per_cu = 13; // VRT_HIP_RENDER_WAVES (1..16): persistent one-wave workgroups per CU: what LDS allows (VGPRs: three
                                  // per SIMD run at a time; the 13th starts when the first retires)
    uint32_t render_grid_override = 0; // VRT_HIP_RENDER_GRID (tests): exactly this many block-kernel workgroups, e.g. ONE wave that drains all work queues
    float cull_ref_n = 4096.f / 3.f; // TileLists::cull_ref_n; VRT_HIP_CULL_REF_N=0: one threshold at every level (round 1)
    int use_chunks = 1;          // VRT_HIP_CHUNKS: 0 every tile tests every Gaussian (rounds 1-2); 1 (default) chunks first for scenes beyond 8192 Gaussians; 2 always
    float cull_prune = 6.f;      // VRT_HIP_CULL_PRUNE: the context's first vrt_hip_ctx::cull_prune
    float table_step = 0.05f;    // VRT_HIP_TABLE_STEP (0..1): the context's first vrt_hip_ctx::table_hx
    float table_budget = 2.5e-5f; // VRT_HIP_TABLE_BUDGET (> 0): the context's first vrt_hip_ctx::table_budget
    float table_room = 0.9f;      // VRT_HIP_TABLE_ROOM (0..10]: share of the budget the kernel's ESTIMATE of its bound may fill when it coarsens the spacing
    float table_adapt = 3.f;      // VRT_HIP_TABLE_ADAPT (1..3): the table kernel may coarsen the requested spacing by up to this factor where its
                                  // estimate of the bound leaves room (1 = never)
    int claim_early = 8;         // CellGrid::claim_early (measured: 2 leaves `-g 16 -w 2048` at 67 us, 8 takes it to 43, "always" costs a 12-waves-per-CU grid 8 % in flight); VRT_HIP_CLAIM_EARLY=0: the block kernel's waves ask for their next block only when they are done with the current one
    bool skip_idle_dense = true; // VRT_HIP_DENSE_SKIP=0: the dense kernel is launched behind every block kernel
    int dense_waves = 16;        // waves per block in the dense kernel (tuning knob: VRT_HIP_DENSE_WAVES = 4 | 8 | 16; 17 = 16 waves without saturation skipping, A/B)
    bool timeline = false;       // VRT_HIP_TIMELINE set: vrt_hip_render prints where the kernels' time goes (print_timeline) ...
    std::string timeline_csv;    // ... and, when its value names a .csv file, writes the raw stamps there
    bool table_diag = false;     // VRT_HIP_TABLE_DIAG set: vrt_hip_render with stats on prints the table phase split
    bool retain_frame = true;    // VRT_HIP_RETAIN_FRAME=0: every vrt_hip_frame clears its whole image (no retained history)
    bool ray_index = false;      // VRT_HIP_RAY_INDEX=1: the context's first vrt_hip_ctx::ray_index
    bool grad_ordered = false;   // VRT_HIP_GRAD_ORDERED=1: the context's first vrt_hip_ctx::grad_ordered
    bool ray_sort = false;       // VRT_HIP_RAY_SORT=1: the context's first vrt_hip_ctx::ray_sort
};

enum TileMode { TILES_NONE = 0, TILES_HOST = 1, TILES_DEVICE = 2 };

// A ray plan (vrt_hip_ray_plan_create*; vrt_hip_rays.cpp): the kept lists of one bundle in device memory of its own, CSR at the caller's
// ray index.  12 B per ray (len, off) and 4 B per kept entry and per long ray; a sorted plan keeps the order and the packed keys as well
// (8 B per ray).  Complete when its creation returns; read by planned bundles on any stream, written by nothing.
struct vrt_hip_ray_plan {
    vrt_hip_ctx *owner = nullptr;
    size_t nrays = 0;
    uint64_t entries = 0, long_rays = 0, scratch_rays = 0, longest = 0;
    bool sorted = false, indexed = false;
    uint32_t scene_n = 0;      // the scene's size, and ...
    uint64_t cull_gen = 0;     // ... vrt_hip_ctx::cull_gen at creation
    uint32_t spheres = 0;      // what a sorted plan's keys were packed for (ray_sort_unpack)
    DevBuf<uint32_t> len, list, long_ids, order, keys;
    DevBuf<unsigned long long> off;
    size_t bytes() const
    {
        return nrays * 12 + (size_t)entries * 4 + (size_t)long_rays * 4 + (sorted ? nrays * 8 : 0);
    }
};

// vrt_hip_ctx::last_stream when nothing is in flight on a caller's stream.  Not nullptr: that is the null stream, which callers do pass
// (torch's default stream), which does not order with the context's non-blocking stream and has to be waited for like any other.
#define VRT_NO_STREAM ((hipStream_t)(intptr_t)-1)
struct vrt_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // the caller's stream the last *_device call enqueued on (may differ from `stream`): state-changing calls wait for
    // it before they touch buffers its kernels may still be reading (quiesce)
    hipStream_t last_stream = VRT_NO_STREAM;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    Tuning tune;

    // counts every change of scene, options or table settings (vrt_hip_state_generation): a holder of mirrored contexts
    // (vrt_hip_group's batch lanes) sees when they are out of date
    uint64_t state_gen = 1;
    // scene (static SoA copy kept so options can be re-applied)
    uint32_t n = 0;
    DevBuf<float> soa[9]; // mu_x mu_y mu_z ar ag ab aa sigma mag
    bool has_alpha = false;
    DevBuf<float4> mu_sig, gA, gB, gC, gD;
    DevBuf<float4> gChunk;       // bounding spheres of every 64 consecutive Gaussians (launch_build_chunks): the tile level tests these first
    DevBuf<uint32_t> iota;
    bool tables_dirty = true;
    bool gA_valid = false;
    // A scene set from device memory (vrt_hip_set_gaussians_device): everything above was filled by kernels on the caller's stream.
    // scene_words: [0..5] the Morton box of the index build, [6] the bits of the scene's largest finite |albedo| above 1 (0: none), which
    // the host has not read while albedo_pending; scene_done is recorded behind the update, scene_order ahead of it on the context's stream.
    bool scene_on_device = false; // the index of this scene is built on the device
    DevBuf<uint32_t> scene_words;
    bool albedo_pending = false;
    hipEvent_t scene_order = nullptr, scene_done = nullptr;
    float gA_origin[3] = { 0, 0, 0 };

    // tiles.  "ref" lists carry the reference semantics (tiles_t): uploaded by the caller (TILES_HOST), one
    // tile holding everything (TILES_NONE), or produced on demand for queries (TILES_DEVICE).  "work" lists
    // are what the render kernel scans: ref lists intersected with the tile-level cull.
    TileMode tile_mode = TILES_NONE;
    float tw = 2.f, th = 2.f;
    uint32_t tiles_w = 1, tiles_h = 1;
    float view[16] = { 0 };
    DevBuf<uint32_t> ref_start, ref_count, ref_indices;
    bool ref_valid = false;
    DevBuf<uint32_t> w_start, w_count, w_indices;
    // frame batches (vrt_hip_frame_batch_device): the context a batch is issued through keeps the argument rows: a ring of pinned host slots and device slots
    static constexpr int BATCH_SLOTS = 4;
    PinnedBuf<vrtk::FrameArgs> batch_host;
    DevBuf<vrtk::FrameArgs> batch_dev;
    size_t batch_cap = 0; // frames per slot
    hipEvent_t batch_copied[BATCH_SLOTS] = {};
    uint32_t batch_seq = 0;
    // retained assembly (vrt_hip_scatter_sparse_retained_device): which cells the buffer's last assembly stored
    struct Retained {
        uint32_t *image = nullptr;
        uint64_t sig = 0;
        uint32_t bg = 0, seq = 0;
        DevBuf<uint32_t> stamp;
    };
    std::vector<Retained> retained; // one history per frame buffer (at most MAX_ASSEMBLY_FRAMES, oldest dropped)
    // tile cones of the list kernel: a function of the rays and the tile geometry only, kept across frames (cone_key =
    // what they were made for)
    DevBuf<float4> tile_cones;
    uint32_t cone_gen = 0;     // tag of the rows made for cone_key's camera (BinArgs::cone_gen)
    std::string cone_key;
    uint32_t plane_gen = 0;
    // cells with at most this many candidates are shaded last (CellGrid::light_threshold; 32 and more file too many cells as light, profiles/r02_experiments.md);
    // lists_light: what the lists now in the buffers were built with (0 for sparse shards and the two-kernel list path)
    static constexpr uint32_t light_cells = 24;
    uint32_t lists_light = 0;
    float albedo_scale = 1.f;    // max(1, largest |albedo| of the scene): divides the prune budget
    float cull_prune;            // vrt_hip_set_cull_prune(): a block-kernel ray may drop the smallest entries of its list while their sum stays below
                                 // cull_prune * cull_ref_n * cull_eps (prune_list; 0 = off).  6: 3 * 6 * 1365 * 1e-9 = 2.46e-5 -- DESIGN.md section 4
    // second level: 32x32-pixel cells of the local tiles + the active / dense queues of the render kernels
    DevBuf<uint32_t> c_count, c_indices, c_active, c_dense, c_dense_sorted, c_scratch, c_overflow, c_counters, c_rq, c_slot;
    uint32_t rq_gen = 0;      // render launches: selects the work-queue counter set (CellGrid::rq)
    uint32_t cells_x = 1, cells_y = 1, cstride = 1, n_cells = 0;
    int lists_for_shard = -1; // sharding mode the cell lists were built for
    uint32_t list_gen = 0;    // list generation: selects the counter set (see cell_grid)
    // dense-launch feedback (CellGrid::feedback): host-mapped, read frames later
    PinnedBuf<volatile uint32_t> h_fb;
    uint32_t *d_fb = nullptr;
    // dense-launch sizing: frame_seq counts render launches; a report in h_fb[3] (the sequence number of the frame
    // that wrote it) newer than reset_seq comes from the current scene / camera / options
    // A camera that moved keeps the reports (an orbit changes the picture gradually) but widens the idle launch until a
    // report from the new pose has arrived (cam_seq): a jump to a pose with dense cells costs one frame at a quarter of
    // the GPU, not one frame on one workgroup.
    uint32_t frame_seq = 0, reset_seq = 0, cam_seq = 0;
    int num_cus = 256;
    float table_hx;               // vrt_hip_set_table_step(): requested node spacing of the table kernel; 0 = the exact kernels only
    float table_budget;           // vrt_hip_set_table_budget(): worst-case change of a ray's radiance the table kernel may cause
    static constexpr int dense_idle_grid = 1; // workgroups of the dense launch when nothing is expected for it: one
                             // 1024-thread workgroup finds a CU with 61 KB of LDS free sooner than eight do (-2 % with frames in flight)
    bool work_is_ref = false; // render straight from the ref lists (no tile-level cull possible)
    bool lists_dirty = true;
    DevBuf<float> xc, yc;
    float grid_tw = 0.f, grid_th = 0.f;
    uint32_t grid_n = 0xFFFFFFFFu;

    // rays
    uint32_t w = 0, h = 0;
    bool plane_mode = false;
    bool view_mode = false;   // rays from inverse(view) (vrt_hip_set_camera_view)
    float inv_view[16] = { 0 };
    bool plane_affine = false; // plane arrays are a pinhole pattern: corner rays bound a tile's cone
    DevBuf<float> xs, ys, zs;
    float cam_pos[3] = { 0, 0, 0 }, cam_right[3] = { 1, 0, 0 }, cam_up[3] = { 0, 1, 0 }, cam_front[3] = { 0, 0, -1 };
    float focal = 1.f;
    bool rays_set = false;

    // options
    int exp_kind = VRT_EXP_VCL, erf_kind = VRT_ERF_AS;
    float cull_eps = 1e-9f;

    // sharding
    int rank = 0, world = 1;
    DevBuf<uint32_t> tile_map, slot_tiles;
    uint32_t n_local = 0, n_slots = 0;
    bool shard_dirty = true;

    // scratch + statistics
    // d_image: the library's own frame buffer (vrt_hip_frame, vrt_hip_render).  Retained between vrt_hip_frame calls: own_stamp[cell]
    // = own_seq of the last frame that lit the cell, valid while own_sig (image size, tile grid, background) stays and nothing else
    // wrote the buffer (own_seq = 0: the next frame clears everything and starts a new history)
    DevBuf<uint32_t> own_stamp;
    uint32_t own_seq = 0;
    struct OwnGeometry { // what a retained history is valid for: compared field by field (a hash of overlapping fields let two tile grids collide)
        uint32_t w = 0, h = 0, tiles_w = 0, tiles_h = 0, tile_w = 0, tile_h = 0, background = 0;
        const uint32_t *image = nullptr;
        bool operator==(const OwnGeometry &o) const
        {
            return w == o.w && h == o.h && tiles_w == o.tiles_w && tiles_h == o.tiles_h && tile_w == o.tile_w && tile_h == o.tile_h &&
                   background == o.background && image == o.image;
        }
    } own_sig;
    // A caller's host frame buffer (vrt_hip_host_register): page-locked and mapped while its holder lives.  history[cell] = 1: the
    // buffer holds that cell of a frame in which it was lit (anything else holds background); valid for `sig` (own_sig without the
    // image pointer) once a delivery with stamps has recorded it.  slot: its word in h_cells (the cells its last finished delivery
    // counted) and its two tally words.  The holder's owner waits for the frames in flight first (quiesce).
    struct HostReg {
        uint32_t *host = nullptr, *dev = nullptr;
        size_t pixels = 0;
        DevBuf<uint8_t> history;
        OwnGeometry sig;
        bool history_valid = false;
        uint32_t slot = 0, launches = 0;
        HostReg() = default;
        HostReg(HostReg &&o) noexcept
            : host(o.host), dev(o.dev), pixels(o.pixels), history(std::move(o.history)), sig(o.sig), history_valid(o.history_valid), slot(o.slot), launches(o.launches)
        {
            o.host = nullptr;
        }
        HostReg &operator=(HostReg &&o) noexcept
        {
            if (this != &o) {
                release();
                host = o.host; dev = o.dev; pixels = o.pixels; history = std::move(o.history); sig = o.sig; history_valid = o.history_valid;
                slot = o.slot; launches = o.launches;
                o.host = nullptr;
            }
            return *this;
        }
        ~HostReg() { release(); }
        void release(); // hipHostUnregister (vrt_hip_host_frame.cpp)
    };
    static constexpr size_t MAX_HOST_BUFFERS = 16;
    std::vector<HostReg> host_regs;
    PinnedBuf<volatile uint32_t> h_cells; // [MAX_HOST_BUFFERS] host-mapped, written by the delivery kernel (HostFrameArgs::cells_out)
    uint32_t *d_cells = nullptr;
    DevBuf<uint32_t> host_tally;          // [2 * MAX_HOST_BUFFERS] HostFrameArgs::tally of each slot
    DevBuf<uint32_t> d_image;
    DevBuf<float4> d_rad;
    // ray bundles (vrt_hip_rays.cpp): the long-ray queue, its two counters, the long kernel's scratch slots and the
    // statistics words grow only; the rays_* buffers stage the host-pointer forms and grow only, each named by what passes through it
    DevBuf<uint32_t> ray_queue, ray_counters, ray_scratch;
    DevBuf<float> gn_work;        // the Gauss-Newton diagonal's long kernel: the running sums of list positions from RAY_LCAP on, a slot per workgroup
    DevBuf<unsigned long long> ray_stats;
    DevBuf<float> rays_in[2];     // origins (one or one per ray), directions
    DevBuf<float> rays_values_in; // a table of values, one for the bundle or one per ray: sample distances, levels
    DevBuf<float> rays_each_in;   // something per ray and value, in: d loss / d radiance [nrays, 4], d loss / d T (or depth) [nrays, ns]
    DevBuf<float> rays_each_out;  // something per ray and value, out: T, depths, d loss / d samples (or levels)
    DevBuf<float> rays_table_out; // the gradient table [n, VRT_HIP_GRAD_STRIDE], cleared ahead of every bundle that adds to it
    DevBuf<float> rays_rows_out;  // the ray rows of a gradient bundle [nrays, VRT_HIP_RAY_GRAD_STRIDE], out
    DevBuf<float> rays_table_in;  // the tangent table of a tangent bundle [n, VRT_HIP_GRAD_STRIDE], in
    DevBuf<float> rays_rows_in;   // the ray tangents of a tangent bundle [nrays, VRT_HIP_RAY_GRAD_STRIDE], in
    DevBuf<float4> rays_rad;      // radiance per ray, out
    DevBuf<uint32_t> rays_img;    // packed pixels per ray, out
    bool ray_stats_valid = false; // ray_stats holds the counts of the last bundle (stats were on for it)
    // Morton index of the ray bundles (vrt_hip_set_ray_index; build_ray_index in vrt_hip_rays.cpp): made with the static tables
    // while it is switched on, or by the first bundle after it was switched on; never per bundle
    bool ray_index = false;       // bundles cull through the index
    bool ray_index_dirty = true;  // the buffers below do not belong to the tables as they are
    DevBuf<uint32_t> ri_perm;     // Morton position -> scene index
    DevBuf<float4> ri_mu_sig, ri_gB, ri_leaves, ri_groups; // permuted rows, spheres over 64 positions, spheres over 64 leaves
    DevBuf<uint32_t> ri_bitmap;   // the long kernel's bitmaps, ceil(n / 32) words per workgroup: zeroed when it grows, left all zero by every bundle
    DevBuf<uint32_t> ri_keys;     // the device build's keys, unsorted and sorted (2 n)
    DevBuf<unsigned char> ri_sort_tmp; // ... and its sort's temporary storage, ri_sort_bytes for a scene of ri_sort_n: grows only
    uint32_t ri_sort_n = 0xFFFFFFFFu;
    size_t ri_sort_bytes = 0;
    bool ray_indexed_last = false; // the last bundle went through the index
    uint32_t ri_last_leaves = 0, ri_last_groups = 0; // ... over this many leaves and groups
    // Ordered gradient tables (vrt_hip_set_grad_ordered; ordered_bundle in vrt_hip_rays.cpp).  Buffers of the context that only grow, used
    // on the stream of the call like the long-ray queue (wait_for_last_stream covers them): per ray the counted length, its records and
    // their first; per record its Gaussian, its ray, its 9 floats, the sorted keys, the consumed order and an identity; per Gaussian where
    // its segment begins and ends; the words of the call; temporary storage of the scan and the sort.
    bool grad_ordered = false;    // gradient bundles with a table take the ordered path
    DevBuf<uint32_t> ord_len, ord_gauss, ord_ray, ord_keys_sorted, ord_order, ord_iota, ord_seg;
    DevBuf<unsigned long long> ord_count, ord_base, ord_words;
    DevBuf<float> ord_rows;
    DevBuf<unsigned char> ord_scan_tmp, ord_sort_tmp;
    size_t ord_iota_filled = 0;   // ord_iota holds 0 .. this - 1
    bool ord_valid = false;       // an ordered call has cleared ord_words: they are that call's
    uint64_t ord_total = 0;       // rows the last ordered call recorded, sentinel rows included (0: it kept nothing, or was refused)
    bool ord_ran = false;         // set by an ordered call that recorded: the host forms look at its mismatch word once they have waited
    // Sorted bundles (vrt_hip_set_ray_sort; sort_bundle in vrt_hip_rays.cpp).  Buffers of the context that only grow, used on the stream of
    // the call like the long-ray queue (wait_for_last_stream covers them): per ray its key, the identity, the sorted keys and the order
    // (slot -> ray id); one word, the rays that keep no sphere; temporary storage of the sort, rs_sort_bytes for a bundle of rs_sort_n rays.
    bool ray_sort = false;        // bundles of more than one wave are shaded in the sorted order
    DevBuf<uint32_t> rs_keys, rs_ids, rs_keys_sorted, rs_order;
    DevBuf<unsigned long long> rs_none;
    DevBuf<unsigned char> rs_sort_tmp;
    size_t rs_sort_n = 0, rs_sort_bytes = 0;
    uint32_t rs_sort_bits = 0;    // ... and keys of this many bits per field (ray_sort_field_bits)
    bool rs_last_valid = false;   // a bundle has run: the two below are its
    bool rs_last_sorted = false;  // it was sorted: rs_keys, rs_order and rs_none are its
    size_t rs_last_rays = 0;
    uint32_t rs_last_spheres = 0; // what its keys were packed for (ray_sort_unpack)
    // Ray plans (vrt_hip_ray_plan_create*, vrt_hip_set_ray_plan; vrt_hip_rays.cpp).  The context owns every plan made through it; the bound
    // one gives every bundle its lists.  cull_gen counts what makes a list stale and nothing else: the Gaussians set again (either
    // setter, vrt_hip_copy_state into this context), cull_eps or the Exp / Erf pair changed -- not the index and sort switches, which
    // state_gen counts too.
    std::vector<vrt_hip_ray_plan *> plans;
    vrt_hip_ray_plan *plan = nullptr; // bound, or nullptr
    int plan_flags = 0;               // VRT_HIP_PLAN_KEEP_LISTS or 0
    uint64_t cull_gen = 1;
    const char *cull_gen_why = "";    // what bumped it last, for the message of a stale plan
    const vrt_hip_ray_plan *rs_last_plan = nullptr; // the last bundle was planned: its order and keys are this plan's
    DevBuf<unsigned long long> d_stats, d_timeline; // d_timeline: VRT_HIP_TIMELINE diagnostics
    size_t timeline_items = 0, timeline_tiles = 0;
    DevBuf<unsigned long long> d_timeline_lists;
    bool stats_on = false;
    vrt_hip_stats last{};
    // kernel timing ring (vrt_hip_enable_kernel_timing)
    static constexpr int TIMING_RING = 512;
    bool timing_on = false;
    std::vector<hipEvent_t> tev; // 4 per slot: before lists, before render, after render, after dense
    bool timing_full = true;
    uint32_t timing_period = 1, timing_frame = 0;
    uint64_t timing_count = 0;
};

int fail(vrt_hip_ctx *c, int code, const std::string &msg); // records msg (c's, or vrt_hip_create's) and returns code

#define HIPCHK(c, call)                                                                            \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail((c), VRT_HIP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

// vrt_hip_api.cpp
int quiesce(vrt_hip_ctx *c);
void wait_for_last_stream(vrt_hip_ctx *c, hipStream_t st); // before work on `st` rewrites what the last frame on another stream may still read
int check_ready(vrt_hip_ctx *c);
int rebuild_tables(vrt_hip_ctx *c);
int build_ray_index(vrt_hip_ctx *c); // vrt_hip_rays.cpp: the tables are built and nothing is in flight
int build_ray_index_device(vrt_hip_ctx *c, hipStream_t st); // vrt_hip_rays.cpp: the same index behind the table build on `st`, nothing waited for
int resolve_albedo_scale(vrt_hip_ctx *c); // albedo_scale of a scene set from device memory, read back once (waits for that update)
int rebuild_shard(vrt_hip_ctx *c);
vrtk::SceneTables tables(const vrt_hip_ctx *c);
vrtk::TileLists tile_geometry(const vrt_hip_ctx *c);
float exp_floor_x(int exp_kind);
bool table_on(const vrt_hip_ctx *c);
int prepare_tile_grid(vrt_hip_ctx *c, float tw, float th);
int ensure_none_ref_lists(vrt_hip_ctx *c);
uint32_t sparse_capacity(vrt_hip_ctx *c); // cells a sparse shard of this context can hold (the same on every rank)
// vrt_hip_frame.cpp
vrtk::BinArgs bin_args(const vrt_hip_ctx *c); // the tile binning's part of a list kernel's arguments
// the frame of vrt_hip_frame into the context's own buffer d_image, on its stream (vrt_hip_frame, vrt_hip_frame_host)
int frame_own_image(vrt_hip_ctx *c, float tw, float th, const float view[16], const float origin[3], int pack_flags);
// vrt_hip_diag.cpp
int ensure_timing_ring(vrt_hip_ctx *c);
int read_stats(vrt_hip_ctx *c);
void print_timeline(vrt_hip_ctx *c);

#pragma GCC visibility pop
