// vrt_hip_assembly.cpp -- frames assembled from the shards of several ranks: compact shards (vrt_hip_assemble_shards*)
// and sparse shards, scattered into a frame buffer that may keep a retained history of which cells it holds
// (vrt_hip_scatter_sparse*).
#include <algorithm>

#include "vrt_hip_ctx.hpp"

using namespace vrtk;

extern "C" {

namespace {
struct AssemblyGeometry {
    TileLists t;
    uint32_t cx, cy, max_cells, frame_cells, bg;
    size_t npix, covered;
    uint64_t sig;
};
int assembly_geometry(vrt_hip_ctx *c, int pack_flags, AssemblyGeometry &g)
{
    int rc = check_ready(c);
    if (rc) return rc;
    g.t = tile_geometry(c);
    if (g.t.tile_w == 0 || g.t.tile_h == 0) return fail(c, VRT_HIP_ERR_INVALID, "scatter_sparse: tile size is 0 pixels");
    g.bg = (pack_flags & VRT_ALPHA_COMPUTED) ? 0u : 0xFF000000u; // what the kernels write where nothing is lit
    // the tiles cover the linear pixel range [0, stride * tile_h * tiles_h) (rt.h:364-365: pix = x + stride * y with the
    // truncated tile size); what lies beyond is written by nobody in a single-GPU frame either and reads 0
    g.npix = (size_t)c->w * c->h;
    g.covered = std::min(g.npix, (size_t)g.t.stride * g.t.tile_h * g.t.tiles_h);
    g.cx = (g.t.tile_w + CELL - 1) / CELL; g.cy = (g.t.tile_h + CELL - 1) / CELL;
    // one workgroup per (shard, slot) up to the shard capacity -- the same on every rank of this context's job
    g.max_cells = sparse_capacity(c);
    g.frame_cells = g.t.tiles_w * g.t.tiles_h * g.cx * g.cy;
    g.sig = ((uint64_t)g.t.tiles_w << 48) ^ ((uint64_t)g.t.tile_w << 32) ^ ((uint64_t)g.t.tile_h << 16) ^ g.t.tiles_h ^ ((uint64_t)c->w << 24) ^
            ((uint64_t)c->h << 8);
    return VRT_HIP_OK;
}
// Background of one frame buffer before its cells are scattered.  Retained: the caller promises that d_image still holds
// what the previous retained assembly of this context left in it; then the 4 B per ray of background (16.8 MB per 2048^2
// frame: ~4 us of HBM writes, more than a rank's share of the rendering at 8 GPUs) shrink to the cells that were lit last
// time and are not now (clear_stale_cells_kernel, after the scatter).  A new buffer, image size, tile grid or background
// value gets the full fill and starts a new history.
// `batch` / `nbatch`: the frame buffers of the call this one belongs to -- their histories' stamp buffers are already part of
// the launch being prepared and must not be evicted to make room (round-2 advisor finding).
int assembly_background(vrt_hip_ctx *c, const AssemblyGeometry &g, uint32_t *d_image, bool retained, hipStream_t st, uint32_t **stamp,
                        uint32_t *seq, bool *incremental, uint32_t *const *batch = nullptr, int nbatch = 0)
{
    *stamp = nullptr; *seq = 0; *incremental = false;
    auto it = std::find_if(c->retained.begin(), c->retained.end(), [&](const vrt_hip_ctx::Retained &r) { return r.image == d_image; });
    if (!retained) {
        if (it != c->retained.end()) { // a plain assembly into a retained buffer ends its history
            // its stamps may still be read by an earlier retained assembly on ANY stream: wait for the device
            HIPCHK(c, hipDeviceSynchronize());
            c->retained.erase(it);
        }
    } else {
        if (it == c->retained.end()) {
            if (c->retained.size() >= (size_t)MAX_ASSEMBLY_FRAMES) {
                // the oldest history that is not one of this call's own buffers (a call has at most MAX_ASSEMBLY_FRAMES
                // distinct buffers and this one is new, so there is one); earlier assemblies of it may have run on another
                // stream than `st`: wait for the device (a rare path: more than 64 frame buffers in rotation)
                auto victim = std::find_if(c->retained.begin(), c->retained.end(), [&](const vrt_hip_ctx::Retained &r) {
                    for (int k = 0; k < nbatch; ++k) if (batch[k] == r.image) return false;
                    return true;
                });
                if (victim == c->retained.end()) return fail(c, VRT_HIP_ERR_INVALID, "scatter_sparse: no retained history can be dropped");
                HIPCHK(c, hipDeviceSynchronize());
                c->retained.erase(victim);
            }
            c->retained.emplace_back();
            it = c->retained.end() - 1;
            it->image = d_image;
        }
        *incremental = it->sig == g.sig && it->bg == g.bg && it->stamp.cap >= g.frame_cells && it->seq != 0 && it->seq != 0xFFFFFFFFu;
        if (!*incremental) {
            HIPCHK(c, it->stamp.reserve(g.frame_cells));
            HIPCHK(c, hipMemsetAsync(it->stamp.p, 0, (size_t)g.frame_cells * sizeof(uint32_t), st));
            it->sig = g.sig; it->bg = g.bg; it->seq = 0;
        }
        *seq = ++it->seq;
        *stamp = it->stamp.p;
    }
    if (!*incremental) {
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)d_image, (int)g.bg, g.covered, st));
        if (g.covered < g.npix) HIPCHK(c, hipMemsetAsync(d_image + g.covered, 0, (g.npix - g.covered) * sizeof(uint32_t), st));
    }
    return VRT_HIP_OK;
}
int scatter_sparse(vrt_hip_ctx *c, const uint32_t *const *d_shards, int nshards, int pack_flags, uint32_t *d_image, void *hip_stream,
                   bool retained)
{
    if (!c || !d_shards || !d_image || nshards < 1 || nshards > MAX_SHARDS) return VRT_HIP_ERR_INVALID;
    AssemblyGeometry g;
    int rc = assembly_geometry(c, pack_flags, g);
    if (rc) return rc;
    ShardPtrs sp{};
    for (int i = 0; i < nshards; ++i) {
        if (!d_shards[i]) return fail(c, VRT_HIP_ERR_INVALID, "scatter_sparse: NULL shard");
        sp.p[i] = d_shards[i];
    }
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t *stamp, seq;
    bool incremental;
    if ((rc = assembly_background(c, g, d_image, retained, st, &stamp, &seq, &incremental))) return rc;
    launch_scatter_sparse(sp, nshards, g.max_cells, d_image, g.t, g.cx, g.cy, c->w, c->h, stamp, seq, st);
    if (incremental) launch_clear_stale_cells(stamp, seq, g.frame_cells, d_image, g.t, g.cx, g.cy, c->w, c->h, g.bg, st);
    HIPCHK(c, hipGetLastError());
    return VRT_HIP_OK;
}
} // namespace

int vrt_hip_assemble_shards_strided_device(vrt_hip_ctx *c, const uint32_t *d_gathered, size_t rank_stride_px,
                                           uint32_t *d_image, void *hip_stream)
{
    if (!c || !d_gathered || !d_image) return VRT_HIP_ERR_INVALID;
    int rc = check_ready(c);
    if (rc) return rc;
    if ((rc = rebuild_shard(c))) return rc;
    const TileLists t = tile_geometry(c);
    if (rank_stride_px < (size_t)c->n_slots * t.tile_w * t.tile_h) return fail(c, VRT_HIP_ERR_INVALID, "assemble: rank stride smaller than one shard");
    launch_assemble(d_gathered, d_image, c->slot_tiles.p, c->n_slots, (uint32_t)c->world, rank_stride_px, t, c->w, c->h,
                    (hipStream_t)hip_stream);
    HIPCHK(c, hipGetLastError());
    return VRT_HIP_OK;
}

int vrt_hip_assemble_shards_device(vrt_hip_ctx *c, const uint32_t *d_gathered, uint32_t *d_image, void *hip_stream)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    return vrt_hip_assemble_shards_strided_device(c, d_gathered, vrt_hip_shard_pixels(c), d_image, hip_stream);
}

int vrt_hip_scatter_sparse_device(vrt_hip_ctx *c, const uint32_t *const *d_shards, int nshards, int pack_flags, uint32_t *d_image,
                                  void *hip_stream)
{
    return scatter_sparse(c, d_shards, nshards, pack_flags, d_image, hip_stream, false);
}
int vrt_hip_scatter_sparse_retained_device(vrt_hip_ctx *c, const uint32_t *const *d_shards, int nshards, int pack_flags,
                                           uint32_t *d_image, void *hip_stream)
{
    return scatter_sparse(c, d_shards, nshards, pack_flags, d_image, hip_stream, true);
}
int vrt_hip_scatter_sparse_batch_device(vrt_hip_ctx *c, const uint32_t *const *d_shards, int nshards, size_t frame_stride_words,
                                        int nframes, int pack_flags, uint32_t *const *d_images, int retained, void *hip_stream)
{
    if (!c || !d_shards || !d_images || nshards < 1 || nshards > MAX_SHARDS) return VRT_HIP_ERR_INVALID;
    if (nframes < 1 || nframes > MAX_ASSEMBLY_FRAMES) return fail(c, VRT_HIP_ERR_INVALID, "scatter_sparse_batch: 1..64 frames per call");
    if (frame_stride_words % 4) return fail(c, VRT_HIP_ERR_INVALID, "scatter_sparse_batch: the frame stride must keep the shards 16-byte aligned");
    AssemblyGeometry g;
    int rc = assembly_geometry(c, pack_flags, g);
    if (rc) return rc;
    ShardPtrs sp{};
    for (int i = 0; i < nshards; ++i) {
        if (!d_shards[i]) return fail(c, VRT_HIP_ERR_INVALID, "scatter_sparse_batch: NULL shard");
        sp.p[i] = d_shards[i];
    }
    hipStream_t st = (hipStream_t)hip_stream;
    AssemblyFrames fr{};
    for (int f = 0; f < nframes; ++f) { // every buffer is looked at before the first one is touched: a rejected call enqueues nothing
        if (!d_images[f]) return fail(c, VRT_HIP_ERR_INVALID, "scatter_sparse_batch: NULL image");
        for (int k = 0; k < f; ++k)
            if (d_images[k] == d_images[f]) return fail(c, VRT_HIP_ERR_INVALID, "scatter_sparse_batch: two frames of a batch into one buffer");
    }
    for (int f = 0; f < nframes; ++f) {
        bool incremental;
        if ((rc = assembly_background(c, g, d_images[f], retained != 0, st, &fr.stamp[f], &fr.seq[f], &incremental, d_images, nframes))) return rc;
        fr.image[f] = d_images[f];
        fr.clear[f] = incremental ? 1 : 0;
    }
    launch_assemble_sparse_batch(sp, nshards, frame_stride_words, fr, nframes, g.max_cells, g.frame_cells, g.t, g.cx, g.cy, c->w, c->h, g.bg, st);
    HIPCHK(c, hipGetLastError());
    return VRT_HIP_OK;
}

} // extern "C"
