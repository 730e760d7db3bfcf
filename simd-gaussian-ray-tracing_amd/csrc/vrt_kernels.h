// vrt_kernels.h -- launch interface between the C-ABI host code (vrt_hip_api.cpp) and the
// gfx950 kernels (the vrt_*kernel*.hip units and vrt_host_frame.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrtk {

constexpr int BLOCK_W = 8;        // one wavefront = one 8x8 pixel block (64 rays)
constexpr int BLOCK_H = 8;
constexpr int CELL = 32;          // second-level cull region: 32x32 pixels = 4x4 blocks
constexpr int TCAP = 1024;        // a tile's candidates kept in LDS by the fused list kernel
constexpr int CH_CAP = 2048;       // chunks of 64 Gaussians a tile may keep after the chunk test (more: every Gaussian is tested, as before round 3)
constexpr int MAX_FUSED_CELLS = 64; // more cells per tile than this: separate cell kernel (one wave per cell)
#ifndef VRT_PCAP
#define VRT_PCAP 96
#endif
#ifndef VRT_PL
#define VRT_PL 24
#endif
constexpr int PCAP = VRT_PCAP;    // per-block candidates cached in LDS (four parameter rows + sigma*mag = 68 B each; 96 since round 3 = the dense threshold: a block of
                                  // this kernel never has more)
#ifndef VRT_DCAP
#define VRT_DCAP 1024
#endif
constexpr int DCAP = VRT_DCAP;        // per-block candidates the dense kernel keeps in LDS (61 KB with the rest; measured: no change below 64 KB, +4 % at 81 KB, +10 % at 104 KB)
constexpr uint32_t ACTIVE_COUNT_SHIFT = 24, ACTIVE_CELL_MASK = 0xFFFFFFu; // CellGrid::active entries: cell id | min(list length, 255) << 24
constexpr int PL = VRT_PL;        // per-lane list capacity (u8 positions into the block's candidates).  A block with a longer per-ray list goes to the
                                  // 16-wave kernels.  Round 4: 24, not 48 -- the pair loops are quadratic in the list length and a block is ONE wave here: a
                                  // block with lists of 40 is 10^5 instructions on a wave that ends up alone on its SIMD, and the launch waits for it
                                  // (`-f cube.obj` 0.59 -> 0.33 ms per frame, teapot 2048^2 5.83 -> 5.63 ms, monkey 4096^2 12.1 -> 11.8 ms; 16 gains nothing
                                  // more and costs the far side of the monkey orbit 2 %: gpurun_out/r04, profiles/r04_experiments.md)

// Device-resident scene tables, 16 B rows for 128-bit (scalar) loads.
struct SceneTables {
    const float4 *mu_sig;   // static: (mu.x, mu.y, mu.z, sigma)
    const float4 *gA;       // per frame: (oc.x, oc.y, oc.z, |oc|^2), oc = mu - origin
    const float4 *gB;       // static: (r = 1/(sqrt2 sigma), 1/(2 sigma^2), K*sigma*mag, cull_x)
    const float4 *gC;       // static: albedo rgba
    const float4 *gD;       // static: (sigma, sigma*mag, mag, 0)
    uint32_t n;
};

struct TileLists {
    const uint32_t *start;    // [ntiles] first entry of tile t in `indices`
    const uint32_t *count;    // [ntiles]
    const uint32_t *indices;
    uint32_t tiles_w, tiles_h;
    uint32_t tile_w, tile_h;  // pixels: (u64)(width*tw/2.f), rt.h:348-349
    uint32_t stride;          // tile_w * tiles_w: the reference's row stride, rt.h:364-365
    // Level-wise cull thresholds (cull_ref_n = 0: one threshold everywhere).  cull_eps bounds what ONE dropped Gaussian
    // could have contributed; what a ray loses is the sum over everything dropped on its way through the levels.  A level
    // that `n` candidates enter (cell level: the tile's work list; block level: the cell's list; ray level: the block's
    // survivors) drops a candidate when its best-case contribution is below cull_eps * cull_ref_n / n, so that the level as a
    // whole loses less than ~3 * cull_ref_n * cull_eps whatever n is: short lists are cut harder, long lists more carefully
    // than with one fixed threshold.  In the tables that is cull_x - ln(cull_ref_n / n).  Thresholds at the Exp floor
    // (`floor_x`: cull_eps = 0, or sigma*mag/cull_eps beyond it) mean "keep unless Exp gives exactly 0" and stay.
    float cull_ref_n;
    float floor_x;
};


// Second-level (cell) candidate lists and the cell queues of the render kernels (empty cells: count == 0, no queue).
struct CellGrid {
    uint32_t cells_x, cells_y;       // cells per tile
    uint32_t cstride;                // capacity of a cell's list slot
    uint32_t *count;                 // [cells]; 0xFFFFFFFF = overflowed its slot: use the tile's list
    uint32_t *indices;               // cell c at indices + c*cstride
    uint32_t n_cells;                // cells of all local tiles
    uint32_t *active;                // cells with short lists (shaded one wavefront per block): cell id | list length << 24 (ACTIVE_COUNT_SHIFT)
    uint32_t *dense;                 // cell ids with long lists: shaded one 16-wave workgroup per block
    uint32_t *scratch;               // dense kernel: cstride words per workgroup (a block's survivors when they outgrow LDS)
    uint32_t *dense_sorted;          // the same, longest list first (order_dense_kernel): the queue order of the dense kernel
    uint32_t *slot;                  // [cells] position of a non-empty cell in its queue (bit 31: the dense queue): its place in
                                     // a sparse shard (RenderTarget::sparse) -- written by the list kernels
    uint32_t *n_active, *n_dense;    // device counters, zeroed before the list kernels add to them
    // Cells with short lists ("light": at most light_threshold candidates -- the rim of what the scene covers) are filed from
    // the BACK of `active` (n_light of them: active[n_cells - 1 - k]) and shaded last: a frame rarely has a multiple of the
    // GPU's wave slots in blocks, and the blocks that run as a fourth wave on their SIMD should be the cheap ones.
    // Raster frames only: a sparse shard needs its cells in one contiguous run of slots (light_threshold = 0 there).
    // (Round 4 tried to queue only the BLOCKS of light cells that some candidate reaches: tools/experiments/light_block_masks.patch.)
    uint32_t *n_light;
    uint32_t light_threshold;
    uint32_t *dense_next;            // work counter of the dense kernel (zeroed with the others)
    uint32_t *overflow, *n_overflow; // blocks (cell*16 + block) whose per-ray lists outgrew the one-wave kernel's
                                     // LDS slots: it hands them to the dense kernel, which runs after it
    uint32_t dense_threshold;        // a cell whose list is longer than this goes to the dense queue
    float prune_budget;              // block kernel: a ray may drop the smallest entries of its list while their sum (units of the tile level's eps) stays below this (prune_list; 0 = off)
    int claim_early;                 // block kernel: a wave claims its next queue entry before it shades the current block when the queues hold at least
                                     // 1/claim_early of the grid size in entries (VRT_HIP_CLAIM_EARLY; 0: never -- after the block, as in rounds 1-2)
    // Launch feedback (host-mapped memory, nullable): [0] = dense cells of the frame, [1] = blocks of its active cells (written by the one-wave kernel),
    // [2] = items (blocks) the dense kernel found in its queues, [3] = sequence number of the frame that wrote [2]
    // The host reads it frames later to SIZE the dense launch: a frame that is expected to have nothing
    // for it gets a handful of workgroups instead of one per CU and no queue sort.  Which kernel shades a block never
    // depends on it.
    uint32_t *feedback;
    uint32_t frame_seq;
    int dense_is_sorted;             // the dense kernel reads dense_sorted (order_dense_kernel ran) or dense (it did not)
    // Work queues of the one-wave kernel: a wave's first block is static (item = wave), the blocks beyond the grid size
    // are pulled from RQ_N counters RQ_STRIDE words apart (item G + q + RQ_N*m is the m-th of queue q).  `rq` is this
    // launch's set (zero on entry), `rq_next` the other set, which this launch clears for the next one.
    uint32_t *rq, *rq_next;
    // table mode (render_table_kernel): requested node spacing in units of 1/r (0 = off) and the largest change of a ray's
    // radiance the table may cause (worst-case bound, checked per ray; a block that fails it is shaded exactly by the same workgroup)
    float table_hx, table_budget;
    float table_room;                // ... and the share of the budget its estimate may fill when it does (the estimate is not the bound)
    float table_adapt;               // the table kernel may choose a spacing up to this many times the requested one where its estimate
                                     // of the error bound leaves room (1 = always as requested)
};
#ifndef VRT_RQ_N
#define VRT_RQ_N 64
#endif
constexpr uint32_t RQ_N = VRT_RQ_N, RQ_STRIDE = 64; // RQ_N <= 64: a wave looks at all counters at once, one per lane

struct RayGen {
    const float *xs, *ys, *zs; // plane arrays (nullptr => basis mode)
    float origin[3];
    float pos[3], right[3], up[3], front[3];
    float focal, inv_half_w, inv_half_h;
    uint32_t width, height;
    // view mode (vrt_hip_set_camera_view): the reference's own plane points, inverse(view) * (x, y, 0, 1) with
    // x = -1 + j / (w/2), y = -1 + i / (h/2) (camera.cpp:60-69), evaluated in glm's order -- bit-identical rays
    int view_mode;
    float m0[3], m1[3], m3[3];  // columns 0, 1, 3 of inverse(view) (column 2 meets the 0 of the point)
    float half_w, half_h;
};

struct RenderTarget {
    uint32_t *image;          // nullable
    float4 *radiance;         // nullable
    int pack_flags;
    // sharding: tile_map[lt] = global tile id of local tile lt (nullptr = identity);
    // compact != 0 => image is the tile-major shard buffer [lt][tile_h][tile_w]
    const uint32_t *tile_map;
    uint32_t n_local_tiles;
    int compact;
    int cleared;              // empty cells were already cleared by the list kernel of this frame
    // Retained frame buffer (vrt_hip_frame's own buffer): `image` still holds the previous frame of this context at this
    // geometry.  stamp[tile * cells per tile + cell] = stamp_seq of the last frame the cell was lit in; the list kernel then
    // clears only the empty cells that were lit in frame stamp_seq - 1 (16 MB of a 2048^2 frame's 18.7 MB of HBM traffic are
    // background written over background otherwise).  nullptr: every empty cell is cleared.
    uint32_t *stamp;
    uint32_t stamp_seq;
    // Sparse shard (multi-GPU transport, vrt_hip_frame_sparse_device): only the 32x32-px cells some Gaussian reaches
    // are stored, cell-major: `image` points at the pixel region, pixel (cx, cy) of the cell in slot s at
    // image[s*1024 + cy*32 + cx]; slot = position in the active queue, or n_active + position in the dense queue.
    // keys[slot] = tile id * cells per tile + cell in tile; sparse_hdr[0] = number of cells.  Empty cells are neither
    // stored nor cleared: whoever assembles the frame fills the background.
    int sparse;
    uint32_t *keys, *sparse_hdr;
    uint32_t sparse_cap;      // capacity (cells) of the shard buffer: header word 1, locates the pixel region
    unsigned long long *stats; // nullable: STAT_WORDS words, indexed by RenderStat below
    unsigned long long *timeline; // nullable diagnostics: 4 wall_clock64 stamps + the hardware id per one-wave work item (5 words)
};
// The words of RenderTarget::stats (the kernels add to them, read_stats() in vrt_hip_diag.cpp turns them into vrt_hip_stats)
enum RenderStat {
    STAT_BLOCK_CANDIDATES = 0,    // survivors of the block culls
    STAT_TILE_ENTRIES = 1,        // list entries the block culls looked at
    STAT_DENSE_OVER_DCAP = 2,     // dense blocks with more than DCAP survivors
    STAT_LANE_ENTRIES = 3,        // block kernel: sum of lane list lengths
    STAT_LANE_MAX_ENTRIES = 4,    // ... sum over blocks of the longest lane list
    STAT_SHADED_BLOCKS = 5,       // ... blocks it shaded
    STAT_DENSE_BLOCKS = 6,        // blocks of the dense path (table kernel and exact body)
    STAT_TABLE_BLOCKS = 7,        // ... of these, by the table kernel
    STAT_DENSE_T_FIRST = 8,       // exact dense kernel, workgroup timeline: earliest start (running minimum) ...
    STAT_DENSE_T_LAST = 9,        // ... latest end,
    STAT_DENSE_BUSY_TICKS = 10,   // ... summed ticks between a workgroup's start and end,
    STAT_DENSE_WORKGROUPS = 11,   // ... workgroups
    STAT_LANE_PAIRS = 12,         // block kernel: sum over rays of (lane list length)^2
    STAT_DENSE_VISITS_FULL = 13,  // exact body: (emitter chunk, absorber) visits evaluated in full,
    STAT_DENSE_VISITS_ZERO = 14,  // ... exactly zero,
    STAT_DENSE_VISITS_COMMON = 15, // ... exactly -2A
    STAT_TABLE_NODES = 16,        // table kernel: sum of node counts over its blocks
    STAT_TABLE_RETRIES = 17,      // ... blocks it did at the reduced spacing
    STAT_TABLE_SKIPS = 18,        // ... (absorber, wave) visits it settled by saturation
    STAT_TABLE_DECLINED = 19,     // ... blocks it declined
    STAT_TABLE_COARSER = 20,      // ... blocks it did at a coarser spacing than requested
    STAT_TABLE_EMPTY = 21,        // ... blocks of its queue that no Gaussian reaches
    STAT_TABLE_NODE_TICKS = 22,   // ... 10-ns ticks in the node loops, summed over waves and blocks
    STAT_TABLE_WAIT_TICKS = 23,   // ... and waiting at the staging groups' barriers
    STAT_TABLE_PHASE = 24,        // ... 10-ns ticks per phase, summed over blocks: eight words (vrt_hip_stats::table_phase_ticks)
    STAT_WORDS = 32
};

void launch_prep_frame(const SceneTables &s, float4 *gA_out, const float origin[3], hipStream_t st);
void launch_build_static(uint32_t n, const float *mu_x, const float *mu_y, const float *mu_z, const float *ar,
                         const float *ag, const float *ab, const float *aa, const float *sigma, const float *mag,
                         float cull_eps, float exp_floor_x, float4 *mu_sig, float4 *gB, float4 *gC, float4 *gD,
                         hipStream_t st);
void launch_render(const SceneTables &s, const TileLists &t, const CellGrid &c, const RayGen &r, const RenderTarget &o,
                   uint32_t grid /* one-wave workgroups */, int exp_kind, int erf_kind, hipStream_t st);
void launch_render_dense(const SceneTables &s, const TileLists &t, const CellGrid &c, const RayGen &r,
                         const RenderTarget &o, uint32_t grid, int dw /* waves per block: 4, 8 or 16 */, int exp_kind,
                         int erf_kind, hipStream_t st);
void launch_order_dense(const CellGrid &c, hipStream_t st);
void launch_render_table(const SceneTables &s, const TileLists &t, const CellGrid &c, const RayGen &r,
                         const RenderTarget &o, uint32_t grid, int exp_kind, int erf_kind, hipStream_t st);
void launch_build_cell_lists(const SceneTables &s, const TileLists &t, const CellGrid &c, const RayGen &r,
                             const uint32_t *tile_map, uint32_t n_cells, int refine, uint32_t *keys, hipStream_t st);

// per-tile list construction: tile binning (rt.cpp:29-69) and/or tile-level cull ("refine")
struct Mat4 { float m[16]; };
struct BinArgs {
    const float4 *mu_sig, *gA, *gB;
    uint32_t n;
    float4 *prep_gA;                 // nullable: the list kernel also writes the per-origin table (centre - origin, squared norm) of ALL Gaussians for the
                                     // kernels behind it -- what prep_frame_kernel does, without its launch; the list kernel itself works from mu_sig
    const float4 *chunks;            // nullable: bounding sphere (centre, radius incl. the members' reach) of every 64 consecutive Gaussians (launch_build_chunks)
    // input: caller-made lists (from_list) ...
    const uint32_t *in_start, *in_count, *in_indices;
    // ... or on-device binning with the reference's test
    Mat4 V;
    const float *xc, *yc;
    float tw, th;
    uint32_t tiles_w;
    // tile-level cull
    int refine;
    RayGen R;
    uint32_t tile_w, tile_h, stride;
    // output: list of tile t at out_indices[out_start[t] ...], length out_count[t]
    const uint32_t *out_start;
    uint32_t *out_indices, *out_count;
    float cull_ref_n, floor_x;       // TileLists::cull_ref_n, floor_x
    // nullable: the tile cones and their cells' cones, two float4 per cone (axis, cos | sin, -, -, -), made by launch_tile_cones for these rays
    // and this tile geometry -- they depend on the camera only, so a frame with the camera of the last one reuses them
    // (otherwise every wave of the workgroup builds the tile's cone itself)
    float4 *tile_cones;
    uint32_t cone_gen;               // a row of tile_cones is valid if it carries this tag (second float4, .y): rows are filled by whoever needs them first --
                                     // the list kernel's workgroups themselves (a camera that moves never pays a table launch) or tile_cones_kernel (batches)
    int cones_known;                 // 0: the camera of this frame is new, no row can carry its tag: do not even read them
    uint32_t cones_cells;            // cells per tile the table holds cones for (row of tile t: t * (1 + cones_cells); 0: tile cones only)
    uint32_t *zero8;                 // nullable: 8 queue counters this launch clears for the kernels after it
    uint32_t *next_zero8;            // nullable: the OTHER counter set, cleared for the next list generation
};
// optional fused second level (see build_tile_lists_kernel)
struct FuseArgs {
    int enabled;
    int do_clear;
    const uint32_t *tile_map;  // local tile -> tile id (nullptr = identity); the grid is over LOCAL tiles
    CellGrid C;
    RenderTarget O;
    unsigned long long *timeline; // nullable diagnostics: 8 wall_clock64 stamps per tile workgroup
};
void launch_build_tile_lists(const BinArgs &a, const FuseArgs &f, bool from_list, uint32_t ntiles, hipStream_t st);
void launch_build_chunks(uint32_t n, const float4 *mu_sig, const float4 *gB, float4 *chunks, hipStream_t st);

// Several frames per launch (vrt_hip_frame_batch_device): what one frame's three kernels take, as a row of a device array;
// the batch variants of the kernels are the same code with blockIdx.y choosing the row.  A frame of a sparse scene is a
// few tens of microseconds of dependent launches: n frames per launch pay the launch gaps and the tails once, and a rank
// that owns an eighth of the tiles still fills its GPU.
struct FrameArgs {
    BinArgs bin; FuseArgs fuse;                                   // list kernel
    SceneTables S; TileLists T; CellGrid C; RayGen R; RenderTarget O;   // one-wave kernel and dense kernel
    // the frame's small set-up kernels, batched too (a launch per frame and member costs more than the work: 512 launches of
    // 14-20 us in a 128-frame orbit on four members, profiles/r03_group.md)
    int do_prep;  float4 *prep_gA; float prep_origin[3];          // prep_frame_kernel: oc = mu - origin, |oc|^2
    int do_cones; uint32_t cones_tiles, cones_cx, cones_cy; float4 *cones_out; // tile_cones_kernel for this frame's camera (bin = its rays and tile geometry)
    int do_order;                                                 // order_dense_kernel
};
void launch_build_tile_lists_batch(const FrameArgs *d_frames, uint32_t nframes, bool from_list, bool chunks, uint32_t ntiles, hipStream_t st);
void launch_render_batch(const FrameArgs *d_frames, uint32_t nframes, uint32_t grid, bool claim, int exp_kind, int erf_kind, hipStream_t st);
void launch_render_dense_batch(const FrameArgs *d_frames, uint32_t nframes, uint32_t grid, int dw, int exp_kind, int erf_kind,
                               hipStream_t st);
// the per-frame set-up kernels of a batch, one launch each: prep_frame (grid.y = frame), tile_cones, order_dense
void launch_frame_setup_batch(const FrameArgs *d_frames, const FrameArgs *h_frames, uint32_t nframes, hipStream_t st);
void launch_order_dense_batch(const FrameArgs *d_frames, const FrameArgs *h_frames, uint32_t nframes, hipStream_t st);
void launch_render_table_batch(const FrameArgs *d_frames, uint32_t nframes, uint32_t grid, uint64_t npix /* of a frame: all the same size */,
                               int exp_kind, int erf_kind, hipStream_t st);
void launch_assemble(const uint32_t *gathered, uint32_t *image, const uint32_t *tile_of_slot, uint32_t slots_per_rank,
                     uint32_t world, uint64_t rank_stride, const TileLists &t, uint32_t width, uint32_t height, hipStream_t st);
void launch_iota(uint32_t *p, uint32_t n, hipStream_t st);
// frame assembly from sparse shards: image = background, then every stored cell of every shard to its place
constexpr int MAX_SHARDS = 64;
struct ShardPtrs { const uint32_t *p[MAX_SHARDS]; };
void launch_scatter_sparse(const ShardPtrs &shards, int nshards, uint32_t max_cells, uint32_t *image, const TileLists &t,
                           uint32_t cells_x, uint32_t cells_y, uint32_t width, uint32_t height, uint32_t *stamp /* nullable */,
                           uint32_t seq, hipStream_t st);
// several frames per assembly launch: per frame its image, its stamps (nullable), its sequence number, and whether the
// stale-cell pass applies (0: the buffer got the full background fill this time)
constexpr int MAX_ASSEMBLY_FRAMES = 64;
struct AssemblyFrames {
    uint32_t *image[MAX_ASSEMBLY_FRAMES];
    uint32_t *stamp[MAX_ASSEMBLY_FRAMES];
    uint32_t seq[MAX_ASSEMBLY_FRAMES];
    uint8_t clear[MAX_ASSEMBLY_FRAMES];
};
void launch_assemble_sparse_batch(const ShardPtrs &shards, int nshards, size_t frame_stride, const AssemblyFrames &frames, int nframes,
                                  uint32_t max_cells, uint32_t n_cells, const TileLists &t, uint32_t cells_x, uint32_t cells_y,
                                  uint32_t width, uint32_t height, uint32_t background, hipStream_t st);
void launch_clear_stale_cells(const uint32_t *stamp, uint32_t seq, uint32_t n_cells, uint32_t *image, const TileLists &t,
                              uint32_t cells_x, uint32_t cells_y, uint32_t width, uint32_t height, uint32_t background, hipStream_t st);
constexpr uint32_t SPARSE_HDR_WORDS = 4; // [0] cells stored, [1] capacity (cells), [2] cells per tile, [3] reserved
__host__ __device__ inline size_t sparse_pixel_offset(uint32_t cap) { return (SPARSE_HDR_WORDS + (size_t)cap + 3) / 4 * 4; }

// Ray bundles (vrt_ray_kernel.hip, vrt_ray_trans_kernel.hip, vrt_ray_depth_kernel.hip, vrt_ray_grad_kernel.hip): caller-given rays, culled per ray, no camera and no tiles.
#ifndef VRT_RAY_PL
#define VRT_RAY_PL 32
#endif
#ifndef VRT_RAY_LCAP
#define VRT_RAY_LCAP 1024
#endif
constexpr int RAY_PL = VRT_RAY_PL;     // per-ray list capacity of the lane = ray kernel (u32 scene indices in LDS, [k*64 + lane]: 8 KB); a ray with a longer
                                       // list goes to the one-wave-per-ray kernel
constexpr int RAY_LCAP = VRT_RAY_LCAP; // survivors the one-wave-per-ray kernel keeps in LDS; beyond that its list continues in its scratch slot
// Where a bundle's kernels take every ray's list from -- a template value of all of them (SRC): the cull against the chunk spheres, the
// same cull through the Morton index (vrt_hip_set_ray_index), or a ray plan's stored lists (vrt_hip_set_ray_plan), which culls nothing
enum RayListSource : int { RAY_LIST_CHUNKS = 0, RAY_LIST_INDEX = 1, RAY_LIST_PLAN = 2 };
struct RayArgs {
    SceneTables S;
    const float4 *chunks;        // bounding spheres of every 64 consecutive Gaussians (launch_build_chunks)
    const float *origins;        // 3 floats per ray (origin_per_ray != 0) or 3 floats in all
    const float *dirs;           // 3 floats per ray, unit length
    int origin_per_ray;
    uint64_t nrays;              // < 2^32: the queue holds ray ids as u32
    float4 *radiance;            // nullable
    uint32_t *image;             // nullable
    int pack_flags;
    uint32_t *queue;             // ids of the rays whose list outgrew RAY_PL
    uint32_t queue_cap;
    uint32_t *counters;          // [0] entries of the queue, [1] the long kernel's work counter; cleared on the stream per call
    uint32_t *scratch;           // S.n words per workgroup of the long kernel
    unsigned long long *stats;   // nullable: rays, short rays, long rays, sum of short list lengths, sum of their squares, chunk tests,
                                 // chunks kept, member tests (per ray: the members its wave visited), long rays that used their scratch slot
    // The Morton index (vrt_hip_set_ray_index; read by the INDEXED instantiations only, nullptr otherwise): the scene's rows in the
    // order of their centres' Morton keys, spheres over every 64 consecutive positions (leaves) and over every 64 consecutive leaves (groups)
    const uint32_t *perm;        // [n] Morton position -> scene index
    const float4 *mu_sig_m, *gB_m; // [n] SceneTables::mu_sig / gB rows in Morton order: the member loops keep their consecutive rows
    const float4 *leaves;        // [ceil(n / 64)] launch_build_chunks over the permuted rows
    const float4 *groups;        // [ceil(leaves / 64)] launch_build_ray_groups
    uint32_t *bitmap;            // ceil(n / 32) words per workgroup of the long kernel, all zero between rays: bit j = scene index j survives
    unsigned long long *index_stats; // nullable: sums over rays of group tests, groups kept, leaf tests, leaves kept (both by the ray's own tests),
                                 // member tests (the members of the leaves its wave visited)
    // Transmittance bundles (vrt_ray_trans_kernel.hip; at the END: the radiance kernels read the offsets they always read)
    const float *s;              // sample distances: ns in all (s_per_ray == 0) or ns per ray, [r * ns + k]
    uint64_t ns;
    int s_per_ray;
    float *T;                    // [r * ns + k]
    // Depth bundles (vrt_ray_depth_kernel.hip; behind everything the other kernels read)
    const float *tau;            // transmittance levels: nt in all (tau_per_ray == 0) or nt per ray, [r * nt + k]
    uint64_t nt;
    int tau_per_ray;
    float *depth;                // [r * nt + k]
    // Gradient bundles (vrt_ray_grad_kernel.hip; behind everything the other kernels read)
    const float4 *grad_radiance; // [r] d(loss) / d(radiance of ray r)
    float *grad;                 // nullable, [S.n * VRT_HIP_GRAD_STRIDE] the caller's table, added to with float atomics; nullptr: no add is issued
    // Transmittance gradient bundles (vrt_ray_trans_grad_kernel.hip; behind everything the other kernels read).  They reuse s, ns,
    // s_per_ray and grad (nullable here).
    const float *grad_T;         // [r * ns + k] d(loss) / d(T[r, k]) (wrt == VRT_HIP_TGRAD_T) or d(loss) / d(depth[r, k]) (VRT_HIP_TGRAD_DEPTH)
    float *grad_s;               // nullable, [r * ns + k], stored: d(loss) / d(s[r, k]) or d(loss) / d(tau[r, k])
    int wrt;
    // Ray gradients (both gradient kernels; behind everything the other kernels read)
    float *grad_rays;            // nullable, [r * VRT_HIP_RAY_GRAD_STRIDE], 16-byte aligned, stored: d(loss) / d(origin), 0, tangential d(loss) / d(dir), 0
    // Ordered gradient tables (vrt_hip_set_grad_ordered; read by the count kernel and the ORDERED instantiations of the gradient kernels
    // only, which never touch `grad`; behind everything the other kernels read)
    uint32_t *ord_len;              // [r] the count pass's list length of ray r, long rays too
    unsigned long long *ord_count;  // [r] the records of ray r: its length, twice that for a long ray when ord_two
    int ord_two;                    // the radiance gradient: a long ray files an emitter and an absorber record per kept Gaussian
    const unsigned long long *ord_base; // [r] the first record of ray r: the exclusive scan of ord_count
    uint32_t *ord_gauss, *ord_ray;  // [record] the Gaussian (S.n: a sentinel row of a ray whose re-cull missed its length) and the ray
    float *ord_rows;                // [record * GRAD_ORD_COLS] the table's columns 0..8
    unsigned long long *ord_words;  // [GRAD_ORD_WORDS]
    // Sorted bundles (vrt_hip_set_ray_sort; behind everything the other kernels read)
    const uint32_t *order;          // nullable, [nrays] slot -> ray id: lane l of workgroup b of a lane = ray kernel takes ray order[64 b + l];
                                    // nullptr: ray 64 b + l, the bundle's own order
    // Tangent bundles (vrt_ray_tangent_kernel.hip; behind everything the other kernels read)
    const float *tangent;           // nullable, [S.n * VRT_HIP_GRAD_STRIDE], 16-byte aligned: the direction's row per Gaussian, columns 9..11 never used
    const float *ray_tangent;       // nullable, [r * VRT_HIP_RAY_GRAD_STRIDE], 16-byte aligned: d origin, -, d direction, - per ray
    float4 *tangent_out;            // [r] stored: how the radiance of ray r moves along the direction
    // Transmittance tangent bundles (vrt_ray_trans_tangent_kernel.hip; behind everything the other kernels read).  They reuse s, ns,
    // s_per_ray, wrt, tangent (columns 4..8 of a row) and ray_tangent.
    const float *s_tangent;         // nullable: d s[r, k] (wrt == VRT_HIP_TGRAD_T) or d tau[r, k] (VRT_HIP_TGRAD_DEPTH), ns in all or [r * ns + k]
    int s_tangent_per_ray;
    float *trans_tangent_out;       // [r * ns + k] stored: how T[r, k], or the depth of level k, moves along the direction
    // Ray plans (vrt_hip_set_ray_plan; read by the RAY_LIST_PLAN instantiations and by the fill pair of vrt_ray_plan_kernel.hip only; behind
    // everything the other kernels read).  CSR at the caller's ray index: ray r keeps pl_entries[pl_off[r] .. pl_off[r] + pl_len[r]),
    // scene indices in ascending order.
    const uint32_t *pl_len;             // [r] the list length of ray r, long rays too
    const unsigned long long *pl_off;   // [r] where its list begins
    const uint32_t *pl_entries;         // the lists
    const uint32_t *pl_long;            // [pl_nlong] the ids of the rays with pl_len > RAY_PL: the long kernel's queue
    uint32_t pl_nlong;
    uint32_t *pl_fill;                  // the fill pair alone: the lists it writes, at pl_off / pl_len of the count pass
    unsigned long long *pl_words;       // the fill pair alone: [RAY_PLAN_WORDS]
    // Gauss-Newton diagonal bundles (vrt_ray_gn_diag_kernel.hip; behind everything the other kernels read).  They reuse grad (the table D
    // is added into; never nullptr here) and the ord_* fields.
    const float4 *gn_weights;           // nullable, [r] the four channel weights of ray r; nullptr: all 1
    float *gn_work;                     // the long kernel's workspace: gn_work_slot floats per workgroup, the running sums of the list
                                        // positions from RAY_LCAP on, [(p - RAY_LCAP) * GN_SUMS + c]; nullptr where S.n <= RAY_LCAP
    uint64_t gn_work_slot;
    uint32_t gn_grid;                   // workgroups of the long kernel: the bundle's long grid, capped by the workspace
};
constexpr int GRAD_ORD_COLS = 9;    // floats per record
constexpr int GN_SUMS = 12;         // the diagonal's running sums per (ray, list position): channel c has 3 c + 0 M (d magnitude), + 1 the coefficient of n, + 2 the sigma sum
// the words of an ordered call, cleared on the stream ahead of its count pass: rays whose re-cull missed the counted length; records
// reduced, Gaussians with records and the longest segment (by the reduction); rows placed, sentinel rows included (by the scan)
enum { GRAD_ORD_MISMATCH = 0, GRAD_ORD_RECORDS = 1, GRAD_ORD_TOUCHED = 2, GRAD_ORD_LONGEST = 3, GRAD_ORD_TOTAL = 4, GRAD_ORD_WORDS = 5 };
// the words of a plan's creation: the count pass's (above; GRAD_ORD_TOTAL = the entries), then the rays with a list longer than RAY_PL,
// those beyond RAY_LCAP, the longest list, and the rays whose fill found another length than the count pass (0, or the plan is refused)
enum { RAY_PLAN_LONG = GRAD_ORD_WORDS, RAY_PLAN_SCRATCH, RAY_PLAN_LONGEST, RAY_PLAN_MISMATCH, RAY_PLAN_WORDS };
constexpr int RAY_STATS_WORDS = 9, RAY_INDEX_STATS_WORDS = 5; // one device buffer: the index's words follow the nine
void launch_ray_bundle(const RayArgs &a, uint32_t long_grid /* one-wave workgroups of the long kernel */, int src /* RayListSource */, int exp_kind, int erf_kind,
                       hipStream_t st);
// the same cull, then T at a.ns sample distances per ray instead of the radiance (vrt_ray_trans_kernel.hip)
void launch_ray_trans_bundle(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
// the same cull, then the distance at which T falls to each of a.nt levels per ray (vrt_ray_depth_kernel.hip)
void launch_ray_depth_bundle(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
// the same cull, then d(loss) / d(Gaussians) from a.grad_radiance, added into a.grad (where there), and d(loss) / d(rays) stored to
// a.grad_rays (where there) (vrt_ray_grad_kernel.hip).  Only the pairs
// ray_grad_pair_supported names have kernels; any other enqueues nothing.
void launch_ray_grad_bundle(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
bool ray_grad_pair_supported(int exp_kind, int erf_kind);
// the same cull, then d(loss) / d(Gaussians) from a.grad_T at the samples a.s, added into columns 4..8 of a.grad, and d(loss) /
// d(samples or levels) stored to a.grad_s, d(loss) / d(rays) to a.grad_rays (vrt_ray_trans_grad_kernel.hip).  The pairs of ray_grad_pair_supported; any other enqueues nothing.
void launch_ray_trans_grad_bundle(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
// the same cull, then J . v: how the radiance of every ray moves along the direction (a.tangent per Gaussian, a.ray_tangent per ray, either
// nullable), stored to a.tangent_out (vrt_ray_tangent_kernel.hip).  The pairs of ray_grad_pair_supported; any other enqueues nothing.
void launch_ray_tangent_bundle(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
// the same cull, then J . v of T at the samples a.s (a.wrt == VRT_HIP_TGRAD_T) or of the depth at the depths a.s (VRT_HIP_TGRAD_DEPTH) along
// the direction (a.tangent, a.ray_tangent, a.s_tangent, each nullable), stored to a.trans_tangent_out (vrt_ray_trans_tangent_kernel.hip).
// The pairs of ray_grad_pair_supported; any other enqueues nothing.
void launch_ray_trans_tangent_bundle(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
// the same cull, then the diagonal of the Gauss-Newton matrix: sum over rays and channels of a.gn_weights times the squared derivative of
// the radiance, added into a.grad (vrt_ray_gn_diag_kernel.hip); _ordered: stored as one record per (ray, kept Gaussian), long rays too
// (vrt_ray_gn_diag_ordered_kernel.hip).  The pairs of ray_grad_pair_supported; any other enqueues nothing.  The long kernel runs on
// min(long_grid, a.gn_grid) workgroups.
void launch_ray_gn_diag_bundle(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
void launch_ray_gn_diag_bundle_ordered(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
// Ordered gradient tables (vrt_hip_set_grad_ordered; vrt_grad_ordered_kernel.hip has the pipeline).  The same two bundles with every
// add into a.grad replaced by a store into the records at a.ord_base[r] (the ORDERED instantiations, in translation units of their own:
// vrt_ray_grad_ordered_kernel.hip, vrt_ray_trans_grad_ordered_kernel.hip); a.grad is not touched.
void launch_ray_grad_bundle_ordered(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
void launch_ray_trans_grad_bundle_ordered(const RayArgs &a, uint32_t long_grid, int src /* RayListSource */, int exp_kind, int erf_kind, hipStream_t st);
// count and place: a.ord_words cleared, a.ord_len / a.ord_count by the cull alone, base = the exclusive scan of a.ord_count (tmp:
// grad_ordered_scan_bytes(nrays) bytes; 0: the query failed), a.ord_words[GRAD_ORD_TOTAL] = the rows of the call.  a.nrays > 0.
size_t grad_ordered_scan_bytes(size_t nrays);
hipError_t launch_grad_ordered_count(const RayArgs &a, int src /* RayListSource */, unsigned long long *base, void *tmp, size_t tmp_bytes, hipStream_t st);
// sort and reduce: `total` records (keys: Gaussian index, n for a sentinel row) into the consumed order, then table[j, first_col..8] +=
// the ordered sum of Gaussian j's records.  sort_tmp: grad_ordered_sort_bytes(total, n) bytes; iota: 0 .. total - 1; seg: 2 n words.
struct GradOrderedSort {
    uint64_t total;
    uint32_t n;
    const uint32_t *keys, *iota;
    uint32_t *keys_sorted, *order, *seg;
    void *sort_tmp;
    size_t sort_bytes;
    const float *rows;
    float *table;
    int first_col; // 0: the radiance gradient, 4: the transmittance gradient (columns 0..3 are not written)
    unsigned long long *words;
};
size_t grad_ordered_sort_bytes(uint64_t total, uint32_t n);
void launch_grad_ordered_iota(uint32_t *p, uint64_t from, uint64_t to, hipStream_t st); // p[i] = i for from <= i < to
hipError_t launch_grad_ordered_reduce(const GradOrderedSort &o, hipStream_t st);
// Sorted bundles (vrt_hip_set_ray_sort; vrt_ray_sort_kernel.hip): keys[r] = the key of ray r by the sphere tests of the cull the bundle
// will run (a.leaves / a.groups with `indexed`, a.chunks without; include/vrt_hip.h states the key), order = the ray ids sorted by
// key, ties in ray order (rocPRIM's stable radix_sort_pairs), *none (cleared on the stream before) = the rays that keep no sphere.
// keys are filed PACKED to the bits the scene's `spheres` (leaves, or chunks: ceil(n / 64)) need -- the same order in fewer radix digits;
// ray_sort_unpack gives the documented key back.  ids: nrays words of scratch (the identity); sort_tmp: ray_sort_bytes(nrays, spheres)
// bytes (0: the query failed).  a.nrays > 0; nothing waits.
struct RaySort {
    uint32_t *keys, *ids, *keys_sorted, *order;
    unsigned long long *none;
    uint32_t spheres;
    void *sort_tmp;
    size_t sort_bytes;
};
size_t ray_sort_bytes(size_t nrays, uint32_t spheres);
uint32_t ray_sort_field_bits(uint32_t spheres);
uint32_t ray_sort_unpack(uint32_t packed, uint32_t spheres);
hipError_t launch_ray_sort(const RayArgs &a, bool indexed, const RaySort &o, hipStream_t st);
// Ray plans (vrt_hip_ray_plan_create*; vrt_ray_plan_kernel.hip).  Behind launch_grad_ordered_count (a.ord_len = a.pl_len, a.ord_two = 0, base =
// a.pl_off: lengths, offsets and the total) launch_ray_plan_info files RAY_PLAN_LONG / _SCRATCH / _LONGEST of `words` (cleared on the stream
// here) from the lengths; launch_ray_plan_fill runs the bundle's cull once more (src: RAY_LIST_CHUNKS or RAY_LIST_INDEX; a.order as the bundle
// would have it) and copies every list to a.pl_fill -- the short kernel its lane's list out of LDS, one wave per long ray (a.queue: the
// plan's, a.queue_cap = the long rays the info pass counted) the LDS and scratch-slot list.  A ray whose length differs from the count pass's
// writes nothing and counts in a.pl_words[RAY_PLAN_MISMATCH].
hipError_t launch_ray_plan_info(const uint32_t *len, uint64_t nrays, unsigned long long *words, hipStream_t st);
void launch_ray_plan_fill(const RayArgs &a, uint32_t long_grid, int src, hipStream_t st);
// group spheres of the Morton index: one per 64 consecutive leaf spheres, bounding them
void launch_build_ray_groups(uint32_t nleaves, const float4 *leaves, float4 *groups, hipStream_t st);

// a scene set from device memory (vrt_scene_kernel.hip)
struct SceneColumns { float *c[9]; }; // mu_x mu_y mu_z ar ag ab aa sigma mag
// the caller's packed rows (mu [n, 3], albedo [n, 4] with alpha in column 3, sigma [n], mag [n]) into the nine columns; *albedo_bits
// (cleared on the stream before) = max(itself, bits of the largest finite |albedo| above 1)
void launch_ingest_scene(uint32_t n, const float *mu, const float *albedo, const float *sigma, const float *mag, const SceneColumns &out,
                         uint32_t *albedo_bits, hipStream_t st);
// The Morton index on the device, morton_order's permutation exactly: perm[Morton position] = scene index and the rows of mu_sig / gB in
// that order.  box: 6 words of scratch; keys: 2 n words; sort_tmp: morton_sort_bytes(n) bytes (0: the query failed); iota: 0 .. n - 1.
size_t morton_sort_bytes(uint32_t n);
hipError_t launch_morton_index(uint32_t n, const float4 *mu_sig, const float4 *gB, const uint32_t *iota, uint32_t *box, uint32_t *keys,
                               void *sort_tmp, size_t sort_bytes, uint32_t *perm, float4 *mu_sig_m, float4 *gB_m, hipStream_t st);
// after launch_build_chunks over the permuted rows: a NaN radius for every leaf with a member that is not finite (build_ray_index's rule)
void launch_morton_open_leaves(uint32_t n, const float4 *mu_sig_m, const float4 *gB_m, float4 *leaves, hipStream_t st);

// point queries
void launch_transmittance(const SceneTables &s, const float o[3], const float n[3], const float *d_s, size_t ns,
                          float *d_T, int exp_kind, int erf_kind, hipStream_t st);
void launch_transmittance_rays(const SceneTables &s, const float *d_origins, const float *d_dirs, const float *d_s,
                               size_t nrays, float *d_T, int exp_kind, int erf_kind, hipStream_t st);
void launch_transmittance_step(const SceneTables &s, const float o[3], const float n[3], const float *d_s, size_t ns,
                               float delta, float *d_T, hipStream_t st);
void launch_density(const SceneTables &s, const float *d_pts, size_t npts, float *d_D, hipStream_t st);
// iota: identity index list 0..n-1 on device
void launch_radiance(const SceneTables &s, const float *d_origins, const float *d_dirs, size_t nrays,
                     const uint32_t *iota, float4 *d_out, int exp_kind, int erf_kind, hipStream_t st);
void launch_eval_erf(int kind, const float *x, size_t n, float *y, hipStream_t st);
void launch_eval_exp(int kind, const float *x, size_t n, float *y, hipStream_t st);

} // namespace vrtk
