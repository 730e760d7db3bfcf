// vrt_kernels.hip -- what a frame sets up before it shades: the scene tables (build_static, prep_frame, iota, build_chunks), the tile
// and cell cones, and the list kernels (tile binning rt.cpp:29-69 + cell lists, fused or as two kernels) with launch_frame_setup_batch.
// Shading, frame assembly and the point queries have units of their own (list: vrt_kernels_common.hpp, which holds what all share).
#include "vrt_kernels_common.hpp"

namespace vrtk {

// ---------------------------------------------------------------------------------------------
// Scene tables
// ---------------------------------------------------------------------------------------------
__global__ void build_static_kernel(uint32_t n, const float *mu_x, const float *mu_y, const float *mu_z,
                                    const float *ar, const float *ag, const float *ab, const float *aa,
                                    const float *sigma, const float *mag, float cull_eps, float exp_floor_x,
                                    float4 *mu_sig, float4 *gB, float4 *gC, float4 *gD)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float s = sigma[i], m = mag[i];
    mu_sig[i] = make_float4(mu_x[i], mu_y[i], mu_z[i], s);
    const float q = s * m;
    // cull_x: drop when d^2/(2 sigma^2) > ln(|q|/eps); never keep what Exp flushes to zero anyway
    float cull_x = exp_floor_x;
    if (q == 0.f) cull_x = -INFINITY;
    else if (cull_eps > 0.f) cull_x = fminf(cull_x, logf(fabsf(q) / cull_eps));
    gB[i] = make_float4(1.f / (SQRT_2 * s), 1.f / (2.f * s * s), q * INV_SQRT_2_PI, cull_x);
    gC[i] = make_float4(ar[i], ag[i], ab[i], aa ? aa[i] : 1.f);
    gD[i] = make_float4(s, q, m, 0.f);
}

void launch_build_static(uint32_t n, const float *mu_x, const float *mu_y, const float *mu_z, const float *ar,
                         const float *ag, const float *ab, const float *aa, const float *sigma, const float *mag,
                         float cull_eps, float exp_floor_x, float4 *mu_sig, float4 *gB, float4 *gC, float4 *gD,
                         hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(build_static_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, mu_x, mu_y, mu_z, ar, ag, ab,
                       aa, sigma, mag, cull_eps, exp_floor_x, mu_sig, gB, gC, gD);
}

__global__ void prep_frame_kernel(uint32_t n, const float4 *mu_sig, float4 *gA, float ox, float oy, float oz)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 m = mu_sig[i];
    const float cx = m.x - ox, cy = m.y - oy, cz = m.z - oz;
    gA[i] = make_float4(cx, cy, cz, dot3_ref(cx, cy, cz, cx, cy, cz)); // vec4f_t::sqnorm order (types.h:69-72)
}

__global__ void prep_frame_batch_kernel(const FrameArgs *__restrict__ frames)
{
    const FrameArgs &a = frames[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!a.do_prep || i >= a.S.n) return;
    const float4 m = a.S.mu_sig[i];
    const float cx = m.x - a.prep_origin[0], cy = m.y - a.prep_origin[1], cz = m.z - a.prep_origin[2];
    a.prep_gA[i] = make_float4(cx, cy, cz, dot3_ref(cx, cy, cz, cx, cy, cz));
}
void launch_prep_frame(const SceneTables &s, float4 *gA_out, const float origin[3], hipStream_t st)
{
    if (!s.n) return;
    hipLaunchKernelGGL(prep_frame_kernel, dim3((s.n + 255) / 256), dim3(256), 0, st, s.n, s.mu_sig, gA_out, origin[0],
                       origin[1], origin[2]);
}

__global__ void iota_kernel(uint32_t *p, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}
void launch_iota(uint32_t *p, uint32_t n, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(iota_kernel, dim3((n + 255) / 256), dim3(256), 0, st, p, n);
}

// ---------------------------------------------------------------------------------------------
// Per-tile Gaussian lists.  One 1024-thread workgroup per reference tile builds, in one pass,
//   (a) the reference's tile set: vrt/rt.cpp:29-69 on device (or takes a caller-made list), and
//   (b) optionally ("refine") drops from it every Gaussian that is below cull_eps for the whole tile
//       (cone through the tile's corner rays), so that the 8x8-block cull of the render kernel
//       scans tens of candidates instead of the reference's ~1600.
// The reference-set arithmetic is kept unfused and in the reference's order so that inclusion
// decisions (a "<=" on floats) reproduce the host algorithm; order of indices is preserved.
// ---------------------------------------------------------------------------------------------
// With F.enabled the same workgroup goes on to the second level: the tile's surviving candidates stay in LDS
// (index + the two parameter rows the cone test reads) and each of its 16 waves filters them for the tile's
// 32x32-pixel cells, files every non-empty cell as active or dense (at most two atomics per TILE) and clears the
// pixels of empty cells on the spot -- no second kernel, no global round trip, no idle clear phase later.
// cone of a whole reference tile, from the centre and the four corner pixels (pinhole rays: the farthest ray of a rectangle
// on the image plane from its centre ray is a corner ray): cell 0 of a one-column grid of cells of 2^32 - 1 pixels, which the clipping
// min(0 + SIZE, tile_w) - 1 turns into the rectangle (0, 0) .. (tile_w - 1, tile_h - 1)
__device__ __forceinline__ Cone tile_cone(const BinArgs &P, uint32_t tx, uint32_t ty, uint32_t lane)
{
    return tile_cell_cone<0xFFFFFFFFu>(P.R, P, tx, ty, 0, 1, lane);
}
// cone of cell ci of a tile (32x32 px, clipped to the tile), as the second level builds it
__device__ __forceinline__ Cone cell_cone(const BinArgs &P, uint32_t tx, uint32_t ty, uint32_t ci, uint32_t cells_x, uint32_t lane)
{
    return tile_cell_cone<CELL>(P.R, P, tx, ty, ci, cells_x, lane);
}
// A row of the cone table: (axis, tag), (cos, sin, tag, -).  The tag (BinArgs::cone_gen) says which camera the row was made for; it sits in
// BOTH halves, so a reader that catches a row between the writer's two stores sees two different tags and takes the row for missing.
__device__ __forceinline__ void cone_row_write(float4 *table, size_t row, const Cone &k, uint32_t gen)
{
    table[2 * row] = make_float4(k.cx, k.cy, k.cz, __uint_as_float(gen));
    table[2 * row + 1] = make_float4(k.cos_t, k.sin_t, __uint_as_float(gen), 0.f);
}
__device__ __forceinline__ bool cone_row_read(const float4 *table, size_t row, uint32_t gen, Cone &k)
{
    const float4 c0 = table[2 * row], c1 = table[2 * row + 1];
    if (__float_as_uint(c0.w) != gen || __float_as_uint(c1.z) != gen) return false;
    k.cx = c0.x; k.cy = c0.y; k.cz = c0.z; k.cos_t = c1.x; k.sin_t = c1.y;
    return true;
}
// One wave per cone: per tile id its own cone (slot 0) and the cones of its cells (slots 1 .. cells per tile) -- what the
// list kernel's workgroups build (and file) themselves when they do not find them; frames of a batch get them from this one launch.
__global__ __launch_bounds__(256) void tile_cones_batch_kernel(const FrameArgs *__restrict__ frames)
{
    const FrameArgs &a = frames[blockIdx.y];
    if (!a.do_cones) return;
    const BinArgs &P = a.bin;
    const uint32_t per = 1 + a.cones_cx * a.cones_cy;
    const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= a.cones_tiles * per) return;
    const uint32_t t = k / per, c = k % per;
    const Cone cn = c ? cell_cone(P, t % P.tiles_w, t / P.tiles_w, c - 1, a.cones_cx, lane) : tile_cone(P, t % P.tiles_w, t / P.tiles_w, lane);
    if (lane == 0) cone_row_write(a.cones_out, k, cn, P.cone_gen);
}
void launch_frame_setup_batch(const FrameArgs *d_frames, const FrameArgs *h_frames, uint32_t nframes, hipStream_t st)
{
    uint32_t n_prep = 0, n_cones = 0;
    for (uint32_t f = 0; f < nframes; ++f) {
        if (h_frames[f].do_prep) n_prep = std::max(n_prep, h_frames[f].S.n);
        if (h_frames[f].do_cones) n_cones = std::max(n_cones, h_frames[f].cones_tiles * (1 + h_frames[f].cones_cx * h_frames[f].cones_cy));
    }
    if (n_prep) hipLaunchKernelGGL(prep_frame_batch_kernel, dim3((n_prep + 255) / 256, nframes), dim3(256), 0, st, d_frames);
    if (n_cones) hipLaunchKernelGGL(tile_cones_batch_kernel, dim3((n_cones + 3) / 4, nframes), dim3(256), 0, st, d_frames);
}

// ---------------------------------------------------------------------------------------------
// Chunk table (round 3): every 64 consecutive Gaussians get a bounding sphere whose radius includes the members' reach -- the distance
// beyond which cone_keeps drops them: x = d^2 / (2 sigma^2) with 0.999 x - 1e-3 > cull_x.  cone_keeps' lower bound of the distance
// between a point and the rays of a cone is 1-Lipschitz in the point, so a cone farther than the radius from the chunk's centre keeps
// none of its members: the tile level then tests N / 64 spheres and the members of the chunks that are left instead of all N Gaussians
// (256 tiles x 4096 x 32 B = 33 MB of L2 reads per `-g 64 -w 2048` frame before: the level ran at L2 bandwidth).  Index order is kept (chunks in
// order, members in order), so the lists are the same lists.  Depends on the scene and cull_eps only: built with the static tables.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void build_chunks_kernel(uint32_t n, const float4 *__restrict__ mu_sig, const float4 *__restrict__ gB, float4 *__restrict__ chunks)
{
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (chunk * 64u >= n) return;
    const uint32_t i = chunk * 64u + lane;
    const bool valid = i < n;
    const float4 p = valid ? mu_sig[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 bq = valid ? gB[i] : make_float4(0.f, 1.f, 0.f, -INFINITY);
    const float lo_x = wave_min(valid ? p.x : INFINITY), hi_x = wave_max(valid ? p.x : -INFINITY);
    const float lo_y = wave_min(valid ? p.y : INFINITY), hi_y = wave_max(valid ? p.y : -INFINITY);
    const float lo_z = wave_min(valid ? p.z : INFINITY), hi_z = wave_max(valid ? p.z : -INFINITY);
    const float mx = 0.5f * (lo_x + hi_x), my = 0.5f * (lo_y + hi_y), mz = 0.5f * (lo_z + hi_z);
    const float dx = p.x - mx, dy = p.y - my, dz = p.z - mz;
    const float xr = bq.w + 1e-3f; // kept iff 0.999 d^2 bq.y - 1e-3 <= cull_x
    const float reach = xr > 0.f ? sqrtf(xr / (0.999f * bq.y)) : 0.f;
    float rho = wave_max(valid ? sqrtf(dx * dx + dy * dy + dz * dz) + reach : 0.f);
    rho = rho * 1.0001f + 1e-6f * (1.f + fabsf(mx) + fabsf(my) + fabsf(mz));
    if (lane == 0) chunks[chunk] = make_float4(mx, my, mz, rho);
}
void launch_build_chunks(uint32_t n, const float4 *mu_sig, const float4 *gB, float4 *chunks, hipStream_t st)
{
    const uint32_t nch = (n + 63u) / 64u;
    if (nch) hipLaunchKernelGGL(build_chunks_kernel, dim3((nch + 3u) / 4u), dim3(256), 0, st, n, mu_sig, gB, chunks);
}
__device__ __forceinline__ bool chunk_keeps(const Cone &k, float4 ch, float ox, float oy, float oz)
{
    const float ax = ch.x - ox, ay = ch.y - oy, az = ch.z - oz;
    const float d2 = ax * ax + ay * ay + az * az;
    const float tc = ax * k.cx + ay * k.cy + az * k.cz;
    const float dperp = __builtin_amdgcn_sqrtf(fmaxf(0.f, d2 - tc * tc - 8e-6f * d2)); // the cancellation's rounding, on the keeping side
    const float dmin = fmaxf(0.f, dperp * k.cos_t - fabsf(tc) * k.sin_t);
    return !(dmin * 0.9999f > ch.w);
}

// What both list kernels file a cell as (the low byte of a flag word in LDS).
enum CellClass : uint32_t { CELL_EMPTY = 0, CELL_ACTIVE = 1, CELL_NONE = 2 /* no such cell */, CELL_DENSE = 3, CELL_LIGHT = 5 };
// class of a cell with a list of `count`.  Only the fused kernel files light cells (`with_light`): they go to the back of the active queue,
// which the unfused kernel's frames do not read from that end.
__device__ __forceinline__ uint32_t cell_class(uint32_t count, const CellGrid &C, bool with_light)
{
    return count ? (count > C.dense_threshold ? CELL_DENSE : (with_light && count <= C.light_threshold ? CELL_LIGHT : CELL_ACTIVE)) : CELL_EMPTY;
}

// ---- the fused list kernel: build_tile_lists_body runs the first level itself and drives the phases below, which share these ----
// what a workgroup knows about itself: its tile (t = frame tile id, lt = launch-local), its threads, the ray origin
struct TileWg { uint32_t t, tx, ty, lt, tid, lane, wave; float org_x, org_y, org_z; };
// the reference's tile rectangle: centre and half extents (rt.cpp:58-59)
struct RefTile { float x, y, ax, ay; };

// the per-origin row of a Gaussian: centre - origin and its squared norm in vec4f_t::sqnorm order (types.h:69-72) -- prep_frame_kernel's arithmetic
__device__ __forceinline__ float4 rel(const TileWg &W, const float4 &m)
{
    const float cx = m.x - W.org_x, cy = m.y - W.org_y, cz = m.z - W.org_z;
    return make_float4(cx, cy, cz, dot3_ref(cx, cy, cz, cx, cy, cz));
}
// (b) the tile's cone: the row an earlier frame with this camera (or tile_cones_batch_kernel) filed, else built and filed here
__device__ __forceinline__ Cone tile_cone_tabled(const BinArgs &P, const TileWg &W)
{
    Cone cone = {};
    bool have = false;
    const size_t row = (size_t)W.t * (1 + P.cones_cells);
    if (P.tile_cones && P.cones_known) have = cone_row_read(P.tile_cones, row, P.cone_gen, cone); // filed by an earlier frame with this camera (or by tile_cones_kernel)
    if (!have) {
        cone = tile_cone(P, W.tx, W.ty, W.lane);
        if (P.tile_cones && W.tid == 0) cone_row_write(P.tile_cones, row, cone, P.cone_gen);
    }
    return cone;
}
// ---- chunk test: one sphere per thread and pass, order-preserving compaction of the chunk ids into s_chunk; returns how many passed ----
__device__ __forceinline__ uint32_t chunk_test(const BinArgs &P, const TileWg &W, const Cone &cone, uint32_t n_in, uint32_t *s_wave_cnt,
                                               uint32_t *s_chunk)
{
    uint32_t n_slots = 0;
    const uint32_t nch = (n_in + 63u) / 64u;
    const float ox = P.R.origin[0], oy = P.R.origin[1], oz = P.R.origin[2];
    for (uint32_t cb = 0; cb < nch; cb += 1024) {
        const uint32_t c = cb + W.tid;
        const bool kc = c < nch && chunk_keeps(cone, P.chunks[c], ox, oy, oz);
        const unsigned long long m = __ballot(kc);
        if (W.lane == 0) s_wave_cnt[W.wave] = (uint32_t)__popcll(m);
        __syncthreads();
        const uint32_t v = W.lane < 16 ? s_wave_cnt[W.lane] : 0u;
        const uint32_t incl = wave_inclusive_sum(v);
        const uint32_t before = lane_value_u32(incl - v, W.wave);
        if (kc) {
            const uint32_t pos = n_slots + before + lane_rank(m);
            if (pos < CH_CAP) s_chunk[pos] = c;
        }
        n_slots += lane_value_u32(incl, 15u);
        __syncthreads();
    }
    return n_slots;
}
// the reference's tile test of one Gaussian (centre and sigma in g), in the reference's operations and order
__device__ __forceinline__ bool ref_tile_keeps(const BinArgs &P, const RefTile &B, const float4 g)
{
#pragma clang fp contract(off)
    // glm mat4*vec4: (m0*v0 + m1*v1) + (m2*v2 + m3*v3), v = (mu, 1)   (rt.cpp:37)
    const float vx = (P.V.m[0] * g.x + P.V.m[4] * g.y) + (P.V.m[8] * g.z + P.V.m[12] * 1.f);
    const float vy = (P.V.m[1] * g.x + P.V.m[5] * g.y) + (P.V.m[9] * g.z + P.V.m[13] * 1.f);
    const float vz = (P.V.m[2] * g.x + P.V.m[6] * g.y) + (P.V.m[10] * g.z + P.V.m[14] * 1.f);
    if (vz < 1.f) return false;              // rt.cpp:38
    const float sig = g.w / vz;              // rt.cpp:40
    if (sig < 1e-5f) return false;           // rt.cpp:41
    const float dx = fabsf(B.x - vx / vz), dy = fabsf(B.y - vy / vz);
    const float s33 = 3.3f * sig;
    return (dx <= B.ax + s33) && (dy <= B.ay + s33); // rt.cpp:58-59
}
// the per-origin table for the render kernels of this frame (this kernel reads none of it): behind everything the frame waits for
__device__ __forceinline__ void write_prep(const BinArgs &P, const TileWg &W)
{
    if (P.prep_gA)
        for (uint32_t i = blockIdx.x * 1024u + W.tid; i < P.n; i += gridDim.x * 1024u) P.prep_gA[i] = rel(W, P.mu_sig[i]);
}
// ---- second level, fused: each wave filters the tile's `total` candidates in LDS with the cones of its cells, writes the cells' lists
//      and counts and leaves class | min(count, 255) << 8 per cell in s_flag ----
__device__ __forceinline__ void filter_cells(const BinArgs &P, const FuseArgs &F, const TileWg &W, uint32_t total, float slack,
                                             const uint32_t *s_idx, const float4 *s_A, const float4 *s_B, uint32_t *s_flag, uint32_t cpt)
{
    const CellGrid &C = F.C;
    for (uint32_t ci = W.wave; ci < cpt; ci += 16) {
        const uint32_t cell = W.lt * cpt + ci;
        uint32_t ctotal = 0;
        if (total > TCAP) {
            ctotal = 0xFFFFFFFFu; // the tile's list did not fit LDS: its cells use the tile list itself
        } else if (total) {
            Cone cc = {};
            if (P.refine) {
                bool have = false;
                const size_t row = (size_t)W.t * (1 + cpt) + 1 + ci;
                const bool tabled = P.tile_cones && P.cones_cells == cpt;
                if (tabled && P.cones_known) have = cone_row_read(P.tile_cones, row, P.cone_gen, cc);
                if (!have) {
                    cc = cell_cone(P, W.tx, W.ty, ci, C.cells_x, W.lane);
                    if (tabled && W.lane == 0) cone_row_write(P.tile_cones, row, cc, P.cone_gen);
                }
            }
            uint32_t *cout = C.indices + (size_t)cell * C.cstride;
            for (uint32_t base = 0; base < total; base += 64) {
                const uint32_t k = base + W.lane;
                bool keep = k < total;
                if (keep && P.refine) {
                    float4 bq = s_B[k];
                    bq.w = slack_cull_x(bq.w, slack, P.floor_x);
                    keep = cone_keeps(cc, s_A[k], bq);
                }
                const unsigned long long mask = __ballot(keep);
                const uint32_t pos = ctotal + lane_rank(mask);
                if (keep && pos < C.cstride) cout[pos] = s_idx[k];
                ctotal += (uint32_t)__popcll(mask);
            }
            if (ctotal > C.cstride) ctotal = 0xFFFFFFFFu;
        }
        if (W.lane == 0) {
            C.count[cell] = ctotal;
            s_flag[ci] = cell_class(ctotal, C, true) | (min(ctotal, 255u) << 8);
        }
    }
}
// ---- filing (wave 0; cpt <= 64: one flag per lane): every non-empty cell into the active, light or dense queue with its slot, stamp and
//      key -- at most three atomics per tile; the empty cells to clear into s_inact, their number into s_base[3] ----
__device__ __forceinline__ void file_cells(const FuseArgs &F, const TileWg &W, const uint32_t *s_flag, uint32_t *s_inact, uint32_t *s_base, uint32_t cpt)
{
    const CellGrid &C = F.C;
    const uint32_t lane = W.lane;
    const uint32_t flag = lane < cpt ? s_flag[lane] : (uint32_t)CELL_NONE;
    const uint32_t mine = flag & 0xFFu, packed_count = (flag >> 8) << ACTIVE_COUNT_SHIFT; // the list length rides in the queue entry
    const unsigned long long m_act = __ballot(mine == CELL_ACTIVE), m_dense = __ballot(mine == CELL_DENSE);
    const unsigned long long m_light = __ballot(mine == CELL_LIGHT);
    // Retained frame buffer (RenderTarget::stamp): the buffer still holds this context's previous frame, so an empty cell
    // needs its 4 KB of background only if it was lit then; a lit cell notes the frame it was lit in.
    bool clear_me = mine == CELL_EMPTY;
    if (F.O.stamp && lane < cpt) {
        uint32_t *stamp = F.O.stamp + (size_t)W.t * cpt + lane;
        if (mine == CELL_EMPTY) clear_me = *stamp == F.O.stamp_seq - 1u;
        else *stamp = F.O.stamp_seq;
    }
    const unsigned long long m_empty = __ballot(clear_me);
    const uint32_t na = (uint32_t)__popcll(m_act), nd = (uint32_t)__popcll(m_dense), nl = (uint32_t)__popcll(m_light);
    // empty cells are not queued (count == 0 says it): most tiles of a sparse frame then add to no counter at all
    uint32_t base_a = 0, base_d = 0, base_l = 0;
    if (lane == 0) {
        if (na) base_a = atomicAdd(C.n_active, na);
        if (nd) base_d = atomicAdd(C.n_dense, nd);
        if (nl) base_l = atomicAdd(C.n_light, nl);
        s_base[3] = (uint32_t)__popcll(m_empty);
    }
    base_a = lane_value_u32(base_a, 0u); base_d = lane_value_u32(base_d, 0u);
    base_l = lane_value_u32(base_l, 0u);
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t cell = W.lt * cpt + lane;
    if (mine == CELL_ACTIVE) {
        const uint32_t pos = base_a + (uint32_t)__popcll(m_act & below);
        C.active[pos] = cell | packed_count;
        if (C.slot) C.slot[cell] = pos;
        if (F.O.sparse) F.O.keys[pos] = W.t * cpt + lane;
    } else if (mine == CELL_LIGHT) { // light: from the back of the active queue (raster frames only: no slot, no key)
        C.active[C.n_cells - 1u - (base_l + (uint32_t)__popcll(m_light & below))] = cell | packed_count;
    } else if (mine == CELL_DENSE) {
        const uint32_t pos = base_d + (uint32_t)__popcll(m_dense & below);
        C.dense[pos] = cell;
        if (C.slot) C.slot[cell] = pos | 0x80000000u;
    } else if (clear_me) {
        s_inact[(uint32_t)__popcll(m_empty & below)] = lane;
    }
}
// ---- clear the cells nothing can reach (the n_inact cells of s_inact): 4 B per ray, most of the frame's HBM traffic.  All 1024 threads,
//      16-byte stores (4 pixels per lane, 512 B per row segment) when the geometry is 4-pixel aligned, else pixel by pixel ----
__device__ __forceinline__ void clear_empty_cells(const BinArgs &P, const FuseArgs &F, const TileWg &W, const uint32_t *s_inact, const uint32_t *s_base, uint64_t npix)
{
    const CellGrid &C = F.C;
    const uint32_t zero_px = (F.O.pack_flags & VRT_ALPHA_COMPUTED) ? 0u : 0xFF000000u;
    const bool wide = F.O.image && !F.O.radiance && (P.tile_w % 4 == 0) && (P.stride % 4 == 0) &&
                      ((uintptr_t)F.O.image % 16 == 0) && (!F.O.compact || (P.tile_w * P.tile_h) % 4 == 0);
    const uint32_t n_inact = s_base[3];
    if (wide) {
        for (uint32_t it = W.tid; it < n_inact * (CELL * CELL / 4); it += 1024) { // one 4-pixel quad per item
            const uint32_t ci = s_inact[it / (CELL * CELL / 4)], q = it % (CELL * CELL / 4);
            const uint32_t pxt = (ci % C.cells_x) * CELL + (q % (CELL / 4)) * 4, pyt = (ci / C.cells_x) * CELL + q / (CELL / 4);
            const uint64_t pix = tile_pixel(P.tile_w, P.tile_h, P.stride, W.tx, W.ty, pxt, pyt);
            if (pxt < P.tile_w && pyt < P.tile_h && pix + 3 < npix) {
                const uint64_t o = F.O.compact ? ((uint64_t)W.lt * P.tile_h + pyt) * P.tile_w + pxt : pix;
                // non-temporal: 16 MB of background per 2048^2 frame that nobody reads again before the host does -- streamed past the
                // L2 instead of ending up as its dirty lines (two frames in flight 20.7 -> 20.1 us, serial frame 31.2 -> 30.9)
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store((u32x4){ zero_px, zero_px, zero_px, zero_px }, reinterpret_cast<u32x4 *>(F.O.image + o));
            }
        }
    } else {
        for (uint32_t it = W.tid; it < n_inact * (CELL * CELL); it += 1024) {
            const uint32_t ci = s_inact[it / (CELL * CELL)], q = it % (CELL * CELL);
            const uint32_t pxt = (ci % C.cells_x) * CELL + q % CELL, pyt = (ci / C.cells_x) * CELL + q / CELL;
            const uint64_t pix = tile_pixel(P.tile_w, P.tile_h, P.stride, W.tx, W.ty, pxt, pyt);
            if (pxt < P.tile_w && pyt < P.tile_h && pix < npix) {
                const uint64_t o = F.O.compact ? ((uint64_t)W.lt * P.tile_h + pyt) * P.tile_w + pxt : pix;
                if (F.O.image) F.O.image[o] = zero_px;
                if (F.O.radiance) F.O.radiance[o] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
}

template <bool FROM_LIST, bool CHUNKS>
__device__ __forceinline__ void build_tile_lists_body(const BinArgs &P, const FuseArgs &F)
{
    static_assert(!(FROM_LIST && CHUNKS), "chunks are runs of consecutive indices: device binning only");
    __shared__ uint32_t s_wave_cnt[64];
    __shared__ uint32_t s_idx[TCAP];
    __shared__ float4 s_A[TCAP], s_B[TCAP];
    __shared__ uint32_t s_flag[MAX_FUSED_CELLS], s_inact[MAX_FUSED_CELLS];
    __shared__ uint32_t s_base[4];
    __shared__ uint32_t s_chunk[CHUNKS ? CH_CAP : 1];
    const uint32_t lt = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t t = F.tile_map ? F.tile_map[lt] : lt;
    const uint32_t tx = t % P.tiles_w, ty = t / P.tiles_w;
    // the queue counters are cleared by the PREVIOUS frame's last kernel or a memset when fusing (this kernel
    // adds to them); the unfused pipeline clears them here for the cell kernel that follows
    if (P.zero8 && !F.enabled && lt == 0 && tid < 8) P.zero8[tid] = 0;
    if (P.next_zero8 && lt == 0 && tid < 8) P.next_zero8[tid] = 0;
    unsigned long long *tl = (F.timeline && tid == 0) ? F.timeline + 8 * (size_t)lt : nullptr;
    if (tl) tl[0] = wall_clock64();
    const float org_x = P.R.origin[0], org_y = P.R.origin[1], org_z = P.R.origin[2];
    const TileWg W = { t, tx, ty, lt, tid, lane, wave, org_x, org_y, org_z };

    RefTile B = { 0.f, 0.f, 0.f, 0.f };
    uint32_t n_in;
    const uint32_t *in_list = nullptr;
    if constexpr (FROM_LIST) {
        n_in = P.in_count[t];
        in_list = P.in_indices + P.in_start[t];
    } else {
#pragma clang fp contract(off)
        n_in = P.n;
        B.x = P.xc[tx]; B.y = P.yc[ty];
        B.ax = fabsf(B.x) + P.tw / 2; B.ay = fabsf(B.y) + P.th / 2; // rt.cpp:58-59 (left-to-right sums)
    }
    uint32_t *out = P.out_indices + P.out_start[t];
    uint32_t total = 0;
    // Four candidates per thread and pass: their rows are requested together (one memory round trip instead of four)
    // and the order-preserving compaction needs one barrier pair per 4096 candidates.  Order = index order:
    // (sub-pass u, wave, lane) lexicographic.
    bool keep[4];
    uint32_t idx[4];
    float4 gb[4], gm[4]; // gm: centre and sigma -- the per-origin row is computed from it (rel), and the reference's tile test needs it anyway
    // chunked: the candidates are the members of the chunks that passed the chunk test, one chunk per (sub-pass, wave) -- the same
    // lexicographic (sub-pass, wave, lane) order as below, which is index order again
    bool chunked = CHUNKS && P.refine && P.chunks != nullptr;
    uint32_t n_slots = 0;
    auto fetch = [&](uint32_t base) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (CHUNKS && chunked) {
                const uint32_t slot = base / 64u + u * 16u + wave;
                idx[u] = slot < n_slots ? s_chunk[slot] * 64u + lane : 0xFFFFFFFFu;
                keep[u] = idx[u] < n_in;
                if (!keep[u]) idx[u] = 0u;
            } else {
                const uint32_t k = base + u * 1024 + tid;
                keep[u] = k < n_in;
                idx[u] = keep[u] ? (FROM_LIST ? in_list[k] : k) : 0u;
            }
            if (keep[u] && (P.refine || F.enabled)) gb[u] = P.gB[idx[u]];
            if (keep[u] && (P.refine || F.enabled || !FROM_LIST)) gm[u] = P.mu_sig[idx[u]];
        }
    };
    if (!CHUNKS || !chunked) fetch(0); // in flight while the cone is set up
    Cone cone = {};
    if (P.refine) cone = tile_cone_tabled(P, W);

    if constexpr (CHUNKS) {
        if (chunked) {
            n_slots = chunk_test(P, W, cone, n_in, s_wave_cnt, s_chunk);
            if (n_slots > CH_CAP) chunked = false; // (wave-uniform) too many chunks for LDS: every Gaussian is a candidate
            fetch(0);
        }
    }
    if (tl) tl[1] = wall_clock64();
    const uint32_t n_cand = (CHUNKS && chunked) ? n_slots * 64u : n_in;
    for (uint32_t base = 0; base < n_cand; base += 4096) {
        if (base) fetch(base);
        unsigned long long mask[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            // The result is (reference tile test) AND (cone test).  The cone test goes first: it is the cheaper
            // one (no divisions) and drops >95 % of the pairs in sparse scenes.
            if (keep[u] && P.refine) keep[u] = cone_keeps(cone, rel(W, gm[u]), gb[u]);
            if constexpr (!FROM_LIST)
                if (keep[u]) keep[u] = ref_tile_keeps(P, B, gm[u]);
            mask[u] = __ballot(keep[u]);
            if (lane == 0) s_wave_cnt[u * 16 + wave] = (uint32_t)__popcll(mask[u]);
        }
        __syncthreads();
        // exclusive prefix over the 64 (sub-pass, wave) counts: one count per lane, wave-level scan
        const uint32_t v = s_wave_cnt[lane];
        const uint32_t incl = wave_inclusive_sum(v);
        const uint32_t excl = incl - v;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t before = lane_value_u32(excl, (uint32_t)u * 16u + wave);
            if (keep[u]) {
                const uint32_t pos = total + before + lane_rank(mask[u]);
                out[pos] = idx[u];
                if (F.enabled && pos < TCAP) { s_idx[pos] = idx[u]; s_A[pos] = rel(W, gm[u]); s_B[pos] = gb[u]; }
            }
        }
        total += lane_value_u32(incl, 63u);
        __syncthreads();
    }
    const float slack = level_slack(P.cull_ref_n, total); // cell level: the tile's work list enters
    if (tid == 0) P.out_count[t] = total;
    if (tl) tl[2] = wall_clock64();
    if (!F.enabled) { write_prep(P, W); return; }

    const uint32_t cpt = F.C.cells_x * F.C.cells_y;
    const uint64_t npix = (uint64_t)P.R.width * P.R.height;
    filter_cells(P, F, W, total, slack, s_idx, s_A, s_B, s_flag, cpt);
    __syncthreads();
    if (tl) tl[3] = wall_clock64();
    if (W.wave == 0) file_cells(F, W, s_flag, s_inact, s_base, cpt);
    __syncthreads();
    if (tl) tl[4] = wall_clock64();
    if (!F.do_clear) { write_prep(P, W); return; }
    clear_empty_cells(P, F, W, s_inact, s_base, npix);
    if (tl) tl[5] = wall_clock64();
    write_prep(P, W);
}
struct ListArgs { BinArgs P; FuseArgs F; };
template <bool FROM_LIST, bool CHUNKS = false>
__global__ __launch_bounds__(1024) void build_tile_lists_kernel(ListArgs) // read through kernel_args<>: vrt_kernels_common.hpp
{
    const ListArgs &a = kernel_args<ListArgs>();
    build_tile_lists_body<FROM_LIST, CHUNKS>(a.P, a.F);
}
template <bool FROM_LIST, bool CHUNKS = false>
__global__ __launch_bounds__(1024) void build_tile_lists_batch_kernel(const FrameArgs *__restrict__ frames)
{
    const FrameArgs &a = frames[blockIdx.y];
    build_tile_lists_body<FROM_LIST, CHUNKS>(a.bin, a.fuse);
}

void launch_build_tile_lists(const BinArgs &a, const FuseArgs &f, bool from_list, uint32_t ntiles, hipStream_t st)
{
    if (!ntiles) return;
    if (from_list) hipLaunchKernelGGL(build_tile_lists_kernel<true>, dim3(ntiles), dim3(1024), 0, st, ListArgs{ a, f });
    else if (a.chunks && a.refine) hipLaunchKernelGGL((build_tile_lists_kernel<false, true>), dim3(ntiles), dim3(1024), 0, st, ListArgs{ a, f });
    else hipLaunchKernelGGL(build_tile_lists_kernel<false>, dim3(ntiles), dim3(1024), 0, st, ListArgs{ a, f });
}
void launch_build_tile_lists_batch(const FrameArgs *d_frames, uint32_t nframes, bool from_list, bool chunks, uint32_t ntiles, hipStream_t st)
{
    if (!ntiles || !nframes) return;
    if (from_list) hipLaunchKernelGGL(build_tile_lists_batch_kernel<true>, dim3(ntiles, nframes), dim3(1024), 0, st, d_frames);
    else if (chunks) hipLaunchKernelGGL((build_tile_lists_batch_kernel<false, true>), dim3(ntiles, nframes), dim3(1024), 0, st, d_frames);
    else hipLaunchKernelGGL(build_tile_lists_batch_kernel<false>, dim3(ntiles, nframes), dim3(1024), 0, st, d_frames);
}

// ---------------------------------------------------------------------------------------------
// Second level: one wavefront per 32x32 pixel cell filters its tile's list with the cell's cone.
// 16 cells share a 1024-thread workgroup so that filing the non-empty cells as active or dense costs
// at most two atomics per 16 cells -- one hot counter word serialises at ~11 ns per returning atomic,
// which 4096 single-cell atomics would turn into the longest kernel.  Empty cells: count == 0, no queue.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void build_cell_lists_kernel(SceneTables S, TileLists T, CellGrid C, RayGen R,
                                                                 const uint32_t *tile_map, uint32_t n_cells, int refine,
                                                                 uint32_t *keys /* sparse shard keys, nullable */)
{
    __shared__ uint32_t s_flag[16];  // a CellClass per wave
    __shared__ uint32_t s_base[3];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t cell = blockIdx.x * 16 + wave;
    uint32_t total = 0;
    if (cell < n_cells) {
        const uint32_t cpt = C.cells_x * C.cells_y;
        const uint32_t lt = cell / cpt, ci = cell % cpt;
        const uint32_t t = tile_map ? tile_map[lt] : lt;
        const uint32_t n_in = T.count[t];
        if (n_in) {
            const uint32_t tx = t % T.tiles_w, ty = t / T.tiles_w;
            Cone cone = {};
            if (refine) cone = tile_cell_cone<CELL>(R, T, tx, ty, ci, C.cells_x, lane);
            const uint32_t *in_list = T.indices + T.start[t];
            uint32_t *out = C.indices + (size_t)cell * C.cstride;
            for (uint32_t base = 0; base < n_in; base += 64) {
                const uint32_t k = base + lane;
                bool keep = false;
                uint32_t idx = 0;
                if (k < n_in) {
                    idx = in_list[k];
                    if (refine) {
                        float4 bq = S.gB[idx];
                        bq.w = slack_cull_x(bq.w, level_slack(T.cull_ref_n, n_in), T.floor_x);
                        keep = cone_keeps(cone, S.gA[idx], bq);
                    } else {
                        keep = true;
                    }
                }
                const unsigned long long mask = __ballot(keep);
                const uint32_t pos = total + lane_rank(mask);
                if (keep && pos < C.cstride) out[pos] = idx;
                total += (uint32_t)__popcll(mask);
            }
        }
        if (lane == 0) C.count[cell] = total > C.cstride ? 0xFFFFFFFFu : total;
    }
    if (lane == 0) s_flag[wave] = cell < n_cells ? cell_class(total, C, false) : (uint32_t)CELL_NONE; // no light class: see cell_class
    const uint32_t packed_count = min(total, 255u) << ACTIVE_COUNT_SHIFT;
    __syncthreads();
    if (tid == 0) {
        uint32_t na = 0, nd = 0;
        for (int w = 0; w < 16; ++w) { na += s_flag[w] == CELL_ACTIVE; nd += s_flag[w] == CELL_DENSE; }
        s_base[0] = na ? atomicAdd(C.n_active, na) : 0u;
        s_base[2] = nd ? atomicAdd(C.n_dense, nd) : 0u;
    }
    __syncthreads();
    if (lane == 0 && cell < n_cells) {
        uint32_t before = 0;
        const uint32_t mine = s_flag[wave];
        for (uint32_t w = 0; w < wave; ++w) before += s_flag[w] == mine;
        if (mine == CELL_ACTIVE) {
            C.active[s_base[0] + before] = cell | packed_count;
            if (C.slot) C.slot[cell] = s_base[0] + before;
            if (keys) {
                const uint32_t cpt = C.cells_x * C.cells_y, lt = cell / cpt;
                keys[s_base[0] + before] = (tile_map ? tile_map[lt] : lt) * cpt + cell % cpt;
            }
        }
        else if (mine == CELL_DENSE) { C.dense[s_base[2] + before] = cell; if (C.slot) C.slot[cell] = (s_base[2] + before) | 0x80000000u; }
    }
}

void launch_build_cell_lists(const SceneTables &s, const TileLists &t, const CellGrid &c, const RayGen &r,
                             const uint32_t *tile_map, uint32_t n_cells, int refine, uint32_t *keys, hipStream_t st)
{
    if (!n_cells) return;
    hipLaunchKernelGGL(build_cell_lists_kernel, dim3((n_cells + 15) / 16), dim3(1024), 0, st, s, t, c, r, tile_map,
                       n_cells, refine, keys);
}
} // namespace vrtk
