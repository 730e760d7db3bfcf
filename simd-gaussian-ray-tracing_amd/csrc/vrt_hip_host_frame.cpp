// vrt_hip_host_frame.cpp -- host frames (include/vrt_hip.h, "host frames"): a caller's host buffer registered once with a
// context, then every frame delivered into it on the context's stream without stopping the GPU.  The reference's operator
// writes each frame into a u32 *image in host memory that its caller allocated once (main.cpp:245, rt.h:344-346, 388-399).
//
// Full or delta.  A delivery writes only the cells that changed in THAT buffer since its last delivery (the kernel of
// vrt_host_frame.hip) when three things hold: the frame kept its per-cell stamps (own_seq != 0 after the render), the
// buffer's history is valid, and the history was recorded for the same image size, tile grid and background.  Anything
// else is one SDMA copy of the whole frame into the buffer, followed by the kernel in history-only mode when there are
// stamps to record.  Histories belong to buffers, not to frames: frames rendered without delivery in between change the
// context's stamps and its own buffer, not what a host buffer holds.
//
// Dense frames.  The kernel writes host memory cell by cell; the SDMA copy moves the whole frame at 56.6 GB/s
// (profiles/host_delivery.md).  Every launch counts the cells a delta writes (after a full copy: the cells lit); the next
// launch on the buffer publishes that count in a host-mapped word per buffer, and a delivery whose buffer's word says more
// than three quarters of the frame's cells is a full copy.  Measured on the cfg5 orbit (monkey 4096^2): a delta whose count
// was above one half took 750 us, the full copy 1186 us, so the two break even above 0.5 * 1186 / 750 = 79 % of the cells.
// The choice lags by two deliveries: launch k publishes the count of launch k - 1, and the host reads the word before it
// enqueues launch k + 1 (with frames in flight it reads an older one still).  Speed only, the pixels are the same either
// way.  A delivery without stamps launches nothing: the two tally words keep their turn.  tests/host_frame_scenes.py models
// all of this word by word.
#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "vrt_hip_ctx.hpp"
#include "vrt_host_frame.h"

using namespace vrtk;

namespace {

// Every registered range of the process, [begin, end) bytes: a buffer belongs to one context at a time.
std::mutex g_ranges_mutex;
std::vector<std::pair<uintptr_t, uintptr_t>> g_ranges;

vrt_hip_ctx::HostReg *find_reg(vrt_hip_ctx *c, const uint32_t *image)
{
    for (auto &r : c->host_regs)
        if (r.host == image) return &r;
    return nullptr;
}

} // namespace

void vrt_hip_ctx::HostReg::release()
{
    if (!host) return;
    if (hipHostUnregister(host) != hipSuccess) (void)hipGetLastError();
    std::lock_guard<std::mutex> lock(g_ranges_mutex);
    const uintptr_t b = (uintptr_t)host;
    g_ranges.erase(std::remove_if(g_ranges.begin(), g_ranges.end(), [b](const std::pair<uintptr_t, uintptr_t> &r) { return r.first == b; }),
                   g_ranges.end());
    host = dev = nullptr;
}

extern "C" {

int vrt_hip_host_register(vrt_hip_ctx *c, uint32_t *image, size_t pixels)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    if (!image || (uintptr_t)image % 64) return fail(c, VRT_HIP_ERR_INVALID, "host_register: image must be a non-NULL, 64-byte aligned pointer");
    if (!pixels || pixels > ((size_t)1 << 40)) return fail(c, VRT_HIP_ERR_INVALID, "host_register: pixels must be in 1 .. 2^40");
    if (c->host_regs.size() >= vrt_hip_ctx::MAX_HOST_BUFFERS)
        return fail(c, VRT_HIP_ERR_INVALID, "host_register: at most 16 host buffers per context");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_cells) { // the per-buffer counts of cells delivered (see "Dense frames" above)
        void *dc = nullptr;
        HIPCHK(c, c->h_cells.alloc(vrt_hip_ctx::MAX_HOST_BUFFERS, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer(&dc, (void *)c->h_cells.p, 0));
        HIPCHK(c, c->host_tally.reserve(2 * vrt_hip_ctx::MAX_HOST_BUFFERS));
        HIPCHK(c, hipMemset(c->host_tally.p, 0, 2 * vrt_hip_ctx::MAX_HOST_BUFFERS * sizeof(uint32_t)));
        c->d_cells = (uint32_t *)dc;
    }
    uint32_t slot = 0;
    while (std::any_of(c->host_regs.begin(), c->host_regs.end(), [slot](const vrt_hip_ctx::HostReg &o) { return o.slot == slot; })) ++slot;
    c->h_cells.p[slot] = 0;
    HIPCHK(c, hipMemset(c->host_tally.p + 2 * slot, 0, 2 * sizeof(uint32_t))); // the slot's last holder was quiesced away
    const uintptr_t b = (uintptr_t)image, e = b + pixels * sizeof(uint32_t);
    std::lock_guard<std::mutex> lock(g_ranges_mutex);
    for (const auto &r : g_ranges)
        if (b < r.second && r.first < e) return fail(c, VRT_HIP_ERR_INVALID, "host_register: the buffer (or part of it) is already registered");
    HIPCHK(c, hipHostRegister(image, pixels * sizeof(uint32_t), hipHostRegisterMapped));
    void *dp = nullptr;
    const hipError_t he = hipHostGetDevicePointer(&dp, image, 0);
    if (he != hipSuccess || !dp || (uintptr_t)dp % 16) {
        (void)hipHostUnregister(image);
        return fail(c, VRT_HIP_ERR_HIP, std::string("host_register: no 16-byte aligned device address for the buffer: ") + hipGetErrorString(he));
    }
    vrt_hip_ctx::HostReg r;
    r.host = image; r.dev = (uint32_t *)dp; r.pixels = pixels; r.slot = slot; // history_valid = false: the first delivery is a full one
    g_ranges.emplace_back(b, e);
    c->host_regs.push_back(std::move(r));
    return VRT_HIP_OK;
}

int vrt_hip_host_unregister(vrt_hip_ctx *c, uint32_t *image)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    vrt_hip_ctx::HostReg *r = find_reg(c, image);
    if (!r) return fail(c, VRT_HIP_ERR_INVALID, "host_unregister: the buffer is not registered with this context");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = quiesce(c); // deliveries in flight write the buffer: it stays registered until they have landed
    if (rc) return rc;
    c->host_regs.erase(c->host_regs.begin() + (r - c->host_regs.data()));
    return VRT_HIP_OK;
}

int vrt_hip_frame_host(vrt_hip_ctx *c, float tw, float th, const float view[16], const float origin[3], int pack_flags,
                       uint32_t *image)
{
    if (!c || !origin || !view) return VRT_HIP_ERR_INVALID;
    // every refusal before anything is enqueued
    vrt_hip_ctx::HostReg *r = find_reg(c, image);
    if (!r) return fail(c, VRT_HIP_ERR_INVALID, "frame_host: the buffer is not registered with this context (vrt_hip_host_register)");
    int rc = check_ready(c);
    if (rc) return rc;
    const size_t npix = (size_t)c->w * c->h;
    if (r->pixels < npix) return fail(c, VRT_HIP_ERR_INVALID, "frame_host: the registered buffer holds fewer pixels than the image");

    if ((rc = frame_own_image(c, tw, th, view, origin, pack_flags))) return rc;

    vrt_hip_ctx::OwnGeometry sig = c->own_sig;
    sig.image = nullptr;
    const uint32_t cx = (sig.tile_w + CELL - 1) / CELL, cy = (sig.tile_h + CELL - 1) / CELL;
    const size_t n_cells = (size_t)sig.tiles_w * sig.tiles_h * cx * cy;
    // own_seq != 0: this frame's list kernel stamped the cells it lit, for the geometry of own_sig
    const bool stamps = c->own_seq != 0 && n_cells > 0 && n_cells <= c->own_stamp.cap;
    const bool dense = (uint64_t)c->h_cells.p[r->slot] * 4 > (uint64_t)n_cells * 3; // a recent delivery counted > 3/4 of the cells
    const bool delta = stamps && r->history_valid && r->sig == sig && r->history.cap >= n_cells && !dense;
    if (!delta) {
        r->history_valid = false;
        HIPCHK(c, hipMemcpyAsync(r->host, c->d_image.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
        if (!stamps) return VRT_HIP_OK; // nothing to record: the next delivery is a full one too
        HIPCHK(c, r->history.reserve(n_cells));
    }
    HostFrameArgs a{};
    a.stamp = c->own_stamp.p; a.seq = c->own_seq; a.history = r->history.p;
    a.image = c->d_image.p; a.host = r->dev;
    a.T.tiles_w = sig.tiles_w; a.T.tiles_h = sig.tiles_h; a.T.tile_w = sig.tile_w; a.T.tile_h = sig.tile_h;
    a.T.stride = sig.tile_w * sig.tiles_w;
    a.cells_x = cx; a.cells_y = cy; a.n_cells = (uint32_t)n_cells; a.width = c->w; a.height = c->h;
    a.background = sig.background;
    a.history_only = delta ? 0 : 1;
    a.tally = c->host_tally.p + 2 * r->slot; a.parity = r->launches++ & 1u; a.cells_out = c->d_cells + r->slot;
    launch_host_frame(a, c->stream);
    HIPCHK(c, hipGetLastError());
    r->sig = sig;
    r->history_valid = true;
    return VRT_HIP_OK;
}

} // extern "C"
