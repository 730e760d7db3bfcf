// vrt_assembly_kernel.hip -- multi-GPU frame assembly: shard buffers into the raster image (assemble, scatter_sparse) and the
// cells a retained image no longer holds back to background (clear_stale_cells); single frame and frame batch.
#include "vrt_kernels_common.hpp"

namespace vrtk {

// scatter rank-major shard buffers [rank](stride rank_stride)[slot][tile_h][tile_w] into the raster image (rt.h:388-399)
__global__ void assemble_kernel(const uint32_t *gathered, uint32_t *image, const uint32_t *tile_of_slot, TileLists T,
                                uint32_t width, uint32_t height, uint32_t slots_per_rank, uint64_t rank_stride)
{
    const uint32_t slot = blockIdx.y;
    const uint32_t t = tile_of_slot[slot];
    if (t == 0xFFFFFFFFu) return;
    const uint32_t *src = gathered + (slot / slots_per_rank) * rank_stride + (size_t)(slot % slots_per_rank) * (T.tile_w * T.tile_h);
    const uint32_t tx = t % T.tiles_w, ty = t / T.tiles_w;
    const uint32_t per_tile = T.tile_w * T.tile_h;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < per_tile; p += gridDim.x * blockDim.x) {
        const uint32_t lx = p % T.tile_w, ly = p / T.tile_w;
        const uint64_t pix = tile_pixel(T.tile_w, T.tile_h, T.stride, tx, ty, lx, ly);
        if (pix < (uint64_t)width * height) image[pix] = src[p];
    }
}

void launch_assemble(const uint32_t *gathered, uint32_t *image, const uint32_t *tile_of_slot, uint32_t slots_per_rank,
                     uint32_t world, uint64_t rank_stride, const TileLists &t, uint32_t width, uint32_t height, hipStream_t st)
{
    const uint32_t n_slots = slots_per_rank * world;
    if (!n_slots) return;
    const uint32_t per_tile = t.tile_w * t.tile_h;
    const uint32_t gx = min((per_tile + 255u) / 256u, 64u);
    hipLaunchKernelGGL(assemble_kernel, dim3(gx ? gx : 1, n_slots), dim3(256), 0, st, gathered, image, tile_of_slot, t,
                       width, height, slots_per_rank, rank_stride);
}

// Frame assembly from sparse shards (multi-GPU): one workgroup per (shard, slot).  The shards may live in another
// GPU's memory (peer access over xGMI): they are read once, 16 B per lane, and only the stored cells travel.
// `stamp` (nullable): per cell of the FRAME (key order), the sequence number of the last assembly that stored it -- see
// clear_stale_cells_kernel.
__device__ __forceinline__ void scatter_sparse_body(const uint32_t *sh, uint32_t max_cells, uint32_t *image, const TileLists &T,
                                                    uint32_t cells_x, uint32_t cells_y, uint32_t width, uint32_t height,
                                                    uint32_t *stamp, uint32_t seq)
{
    const uint32_t slot = blockIdx.x, n = sh[0], cap = sh[1];
    if (cap != max_cells || sh[2] != cells_x * cells_y) return; // not a shard of this job's geometry: touch nothing
    if (slot >= n || slot >= max_cells) return;
    const uint32_t cpt = cells_x * cells_y;
    const uint32_t key = sh[SPARSE_HDR_WORDS + slot];
    const uint32_t t = key / cpt, ci = key % cpt;
    if (t >= T.tiles_w * T.tiles_h) return;
    const uint32_t tx = t % T.tiles_w, ty = t / T.tiles_w;
    if (stamp && threadIdx.x == 0) stamp[key] = seq;
    const uint4 *src = reinterpret_cast<const uint4 *>(sh + sparse_pixel_offset(cap) + (size_t)slot * (CELL * CELL));
    const uint64_t npix = (uint64_t)width * height;
    for (uint32_t q = threadIdx.x; q < CELL * CELL / 4; q += blockDim.x) { // one 4-pixel quad per lane and pass
        const uint4 v = src[q];
        const uint32_t cx = (q % (CELL / 4)) * 4, cy = q / (CELL / 4);
        const uint32_t pxt = (ci % cells_x) * CELL + cx, pyt = (ci / cells_x) * CELL + cy;
        if (pyt >= T.tile_h) continue;
        const uint64_t pix = tile_pixel(T.tile_w, T.tile_h, T.stride, tx, ty, pxt, pyt);
        const uint32_t px[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (pxt + k < T.tile_w && pix + k < npix) image[pix + k] = px[k];
    }
}

__global__ __launch_bounds__(256) void scatter_sparse_kernel(ShardPtrs shards, uint32_t max_cells, uint32_t *image, TileLists T,
                                                             uint32_t cells_x, uint32_t cells_y, uint32_t width, uint32_t height,
                                                             uint32_t *stamp, uint32_t seq)
{
    scatter_sparse_body(shards.p[blockIdx.y], max_cells, image, T, cells_x, cells_y, width, height, stamp, seq);
}
// several frames per launch (blockIdx.z): frame f's shard s starts frame_stride words behind frame f-1's
__global__ __launch_bounds__(256) void scatter_sparse_batch_kernel(ShardPtrs shards, size_t frame_stride, AssemblyFrames F,
                                                                   uint32_t max_cells, TileLists T, uint32_t cells_x, uint32_t cells_y,
                                                                   uint32_t width, uint32_t height)
{
    const uint32_t f = blockIdx.z;
    scatter_sparse_body(shards.p[blockIdx.y] + f * frame_stride, max_cells, F.image[f], T, cells_x, cells_y, width, height,
                        F.stamp[f], F.seq[f]);
}

// Retained frames: an image buffer that still holds the previous assembly needs no background fill -- only the cells that
// were stored last time and are not stored now go back to background.  One wave per cell of the frame: stamp == seq - 1
// means "stored by the previous assembly, not by this one" (the scatter kernel of this assembly ran before this kernel).
__device__ __forceinline__ void clear_stale_cells_body(const uint32_t *stamp, uint32_t seq, uint32_t n_cells, uint32_t *image,
                                                       const TileLists &T, uint32_t cells_x, uint32_t cells_y, uint32_t width,
                                                       uint32_t height, uint32_t background)
{
    // one cell per LANE to look at (a frame has thousands of cells and a handful of stale ones), the wave then clears the
    // stale ones of its 64 one after the other
    const uint32_t lane = threadIdx.x & 63, key0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (!stamp || key0 >= n_cells) return;
    const uint32_t mine = key0 + lane;
    unsigned long long stale = __ballot(mine < n_cells && stamp[mine] == seq - 1);
    const uint32_t cpt = cells_x * cells_y;
    const uint64_t npix = (uint64_t)width * height;
    while (stale) {
        const uint32_t key = key0 + (uint32_t)__builtin_ctzll(stale);
        stale &= stale - 1;
        const uint32_t t = key / cpt, ci = key % cpt;
        const uint32_t tx = t % T.tiles_w, ty = t / T.tiles_w;
        for (uint32_t q = lane; q < CELL * CELL; q += 64) {
            const uint32_t pxt = (ci % cells_x) * CELL + q % CELL, pyt = (ci / cells_x) * CELL + q / CELL;
            const uint64_t pix = tile_pixel(T.tile_w, T.tile_h, T.stride, tx, ty, pxt, pyt);
            if (pxt < T.tile_w && pyt < T.tile_h && pix < npix) image[pix] = background;
        }
    }
}
__global__ __launch_bounds__(256) void clear_stale_cells_kernel(const uint32_t *stamp, uint32_t seq, uint32_t n_cells, uint32_t *image,
                                                                TileLists T, uint32_t cells_x, uint32_t cells_y, uint32_t width,
                                                                uint32_t height, uint32_t background)
{
    clear_stale_cells_body(stamp, seq, n_cells, image, T, cells_x, cells_y, width, height, background);
}
// blockIdx.y = frame; frames whose buffer got the full fill this time carry clear[f] = 0
__global__ __launch_bounds__(256) void clear_stale_cells_batch_kernel(AssemblyFrames F, uint32_t n_cells, TileLists T, uint32_t cells_x,
                                                                      uint32_t cells_y, uint32_t width, uint32_t height,
                                                                      uint32_t background)
{
    const uint32_t f = blockIdx.y;
    if (!F.clear[f]) return;
    clear_stale_cells_body(F.stamp[f], F.seq[f], n_cells, F.image[f], T, cells_x, cells_y, width, height, background);
}

void launch_scatter_sparse(const ShardPtrs &shards, int nshards, uint32_t max_cells, uint32_t *image, const TileLists &t,
                           uint32_t cells_x, uint32_t cells_y, uint32_t width, uint32_t height, uint32_t *stamp, uint32_t seq,
                           hipStream_t st)
{
    if (nshards <= 0 || !max_cells) return;
    hipLaunchKernelGGL(scatter_sparse_kernel, dim3(max_cells, (uint32_t)nshards), dim3(256), 0, st, shards, max_cells, image, t,
                       cells_x, cells_y, width, height, stamp, seq);
}
void launch_assemble_sparse_batch(const ShardPtrs &shards, int nshards, size_t frame_stride, const AssemblyFrames &frames, int nframes,
                                  uint32_t max_cells, uint32_t n_cells, const TileLists &t, uint32_t cells_x, uint32_t cells_y,
                                  uint32_t width, uint32_t height, uint32_t background, hipStream_t st)
{
    if (nshards <= 0 || nframes <= 0 || !max_cells) return;
    // a frame stride shorter than a whole shard (a gathered prefix) cannot hold more cells than fit in it: no workgroups for
    // slots that did not travel
    uint32_t slots = max_cells;
    const size_t hdr = sparse_pixel_offset(max_cells);
    if (frame_stride > hdr && frame_stride < hdr + (size_t)max_cells * (CELL * CELL))
        slots = (uint32_t)std::max<size_t>(1, (frame_stride - hdr) / (CELL * CELL));
    hipLaunchKernelGGL(scatter_sparse_batch_kernel, dim3(slots, (uint32_t)nshards, (uint32_t)nframes), dim3(256), 0, st, shards,
                       frame_stride, frames, max_cells, t, cells_x, cells_y, width, height);
    bool any = false;
    for (int f = 0; f < nframes; ++f) any = any || frames.clear[f];
    if (any && n_cells)
        hipLaunchKernelGGL(clear_stale_cells_batch_kernel, dim3((n_cells + 255) / 256, (uint32_t)nframes), dim3(256), 0, st, frames, n_cells, t,
                           cells_x, cells_y, width, height, background);
}
void launch_clear_stale_cells(const uint32_t *stamp, uint32_t seq, uint32_t n_cells, uint32_t *image, const TileLists &t,
                              uint32_t cells_x, uint32_t cells_y, uint32_t width, uint32_t height, uint32_t background, hipStream_t st)
{
    if (!n_cells) return;
    hipLaunchKernelGGL(clear_stale_cells_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, st, stamp, seq, n_cells, image, t, cells_x,
                       cells_y, width, height, background);
}
} // namespace vrtk
