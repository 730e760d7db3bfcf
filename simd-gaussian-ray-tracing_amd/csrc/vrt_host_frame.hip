// vrt_host_frame.hip -- frame delivery into a caller's host buffer (vrt_hip_frame_host, include/vrt_hip.h "host frames").
// The buffer is page-locked and mapped (vrt_hip_host_register), so the kernel stores straight into host memory over the
// host link.  It writes only what changed since the buffer last received a frame: the cells lit now (copied from the
// device frame) and the cells lit at that delivery that are dark now (background).  Everything else in the buffer already
// holds this frame's pixels.  The rest of the frame pipeline stays as it is: this unit only reads its buffers.
#include "vrt_host_frame.h"
#include "vrt_kernels_common.hpp"

namespace vrtk {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One cell's rectangle into host memory: its pixels (lit) or the background.  A row of a cell is 8 lanes x 16 B = one
// 128-byte segment; a pass covers 8 rows, four passes the cell.  Host memory is written by non-temporal stores (nothing
// re-reads it on the GPU).  Rows that are not 16-byte aligned (tile width not a multiple of 4) go out as dwords.
__device__ __forceinline__ void deliver_cell(HostFrameArgs a, uint32_t key, uint32_t lane, bool lit)
{
    // cell key -> raster rectangle, as scatter_sparse_body (vrt_assembly_kernel.hip) maps it
    const uint32_t cpt = a.cells_x * a.cells_y;
    const uint32_t t = key / cpt, ci = key % cpt;
    const uint32_t tx = t % a.T.tiles_w, ty = t / a.T.tiles_w;
    const uint64_t npix = (uint64_t)a.width * a.height;
    const uint32_t pxt = (ci % a.cells_x) * CELL + (lane % 8) * 4;
    if (pxt >= a.T.tile_w) return; // columns of a partial cell beyond its tile
    // tile_w % 4 == 0 makes stride and every quad's first pixel multiples of 4; npix % 4 == 0 makes a quad that starts in
    // the image end in it
    const bool vec = a.T.tile_w % 4 == 0 && npix % 4 == 0;
    const u32x4 bg4 = { a.background, a.background, a.background, a.background };
    for (uint32_t row = lane / 8; row < CELL; row += 8) {
        const uint32_t pyt = (ci / a.cells_x) * CELL + row;
        if (pyt >= a.T.tile_h) break;
        const uint64_t pix = tile_pixel(a.T.tile_w, a.T.tile_h, a.T.stride, tx, ty, pxt, pyt);
        if (vec) {
            if (pix >= npix) break;
            const u32x4 v = lit ? *reinterpret_cast<const u32x4 *>(a.image + pix) : bg4;
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(a.host + pix));
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (pxt + k < a.T.tile_w && pix + k < npix) __builtin_nontemporal_store(lit ? a.image[pix + k] : a.background, a.host + pix + k);
        }
    }
}

// One wave per cell: the decision is the cell's (wave-uniform), and the cells a delivery writes (a few hundred, next to each
// other) go out in parallel.  Each workgroup that writes adds its count of cells to tally[parity]; workgroup 0 publishes
// the other word -- the complete count of the previous launch on this buffer (launches on one buffer run one after the
// other, on one stream) -- in host memory and clears it for the next launch.
__global__ __launch_bounds__(256) void host_frame_kernel(HostFrameArgs a)
{
    __shared__ uint32_t s_cells[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, key = blockIdx.x * 4 + wave;
    bool counted = false;
    if (key < a.n_cells) {
        const bool lit = a.stamp[key] == a.seq;
        const bool held = a.history[key] != 0;
        if (lane == 0) a.history[key] = lit ? 1 : 0;
        counted = lit || (held && !a.history_only);
        if (!a.history_only && counted) deliver_cell(a, key, lane, lit);
    }
    if (lane == 0) s_cells[wave] = counted ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n = s_cells[0] + s_cells[1] + s_cells[2] + s_cells[3];
        if (n) atomicAdd(&a.tally[a.parity], n);
        if (blockIdx.x == 0) *a.cells_out = atomicExch(&a.tally[a.parity ^ 1u], 0u);
    }
}

} // namespace

void launch_host_frame(const HostFrameArgs &a, hipStream_t st)
{
    if (!a.n_cells) return;
    hipLaunchKernelGGL(host_frame_kernel, dim3((a.n_cells + 3) / 4), dim3(256), 0, st, a);
}

} // namespace vrtk
