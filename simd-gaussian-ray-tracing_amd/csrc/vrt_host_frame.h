// vrt_host_frame.h -- launch interface of the host-frame delivery kernel (vrt_host_frame.hip): a frame of the context's own
// buffer written into a caller's registered (page-locked, mapped) host buffer, only the cells that changed since that
// buffer last received a frame (vrt_hip_frame_host in include/vrt_hip.h; host side in vrt_hip_host_frame.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vrt_kernels.h"

namespace vrtk {

struct HostFrameArgs {
    const uint32_t *stamp;    // [n_cells] the context's own_stamp: stamp == seq <=> the list kernel of this frame lit the cell
    uint32_t seq;             // own_seq of the frame in `image`
    uint8_t *history;         // [n_cells] the host buffer's history: 1 = the buffer holds a lit cell there (not background)
    const uint32_t *image;    // the frame on the device (raster order, w * h)
    uint32_t *host;           // device address of the registered host buffer (hipHostGetDevicePointer), 16-byte aligned
    TileLists T;              // tiles_w, tiles_h, tile_w, tile_h, stride only
    uint32_t cells_x, cells_y, n_cells, width, height;
    uint32_t background;      // what a dark cell holds
    int history_only;         // 1: record history = lit now, write no pixel (the buffer just got a full copy)
    uint32_t *tally;          // [2] device words: this launch adds its cells to tally[parity] and publishes (then clears) the other
    uint32_t parity;          // the buffer's launch count & 1
    uint32_t *cells_out;      // device address of a mapped host word: the count of the buffer's PREVIOUS launch of cells a delta
                              // writes (lit now, or held and dark now; after a full copy: lit now)
};

// One wave per cell, four cells per 256-thread workgroup; on `st`.
void launch_host_frame(const HostFrameArgs &a, hipStream_t st);

} // namespace vrtk
