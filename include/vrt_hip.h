/*
 * vrt_hip.h -- C ABI of libvrt_hip.so: the MI355X (gfx950) implementation of the
 * reference's render / radiance / transmittance path.
 *
 * The reference has no FFI layer: the path is a set of C++ header templates in
 * namespace vrt (src/vrt/rt.h:16-405) instantiated by its callers
 * (src/volumetric-ray-tracer/main.cpp:271-292, tests/transmittance.cpp:27-30,
 * tests/img-error.cpp:34-43).  Each entry point below names the reference
 * interface it replaces.  The C++ header include/vrt/vrt.hpp re-creates the
 * vrt:: signatures on top of this ABI; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - every function returns VRT_HIP_OK (0) or a negative vrt_hip_status; nothing
 *     exits the process (the reference _exit(1)s, include/definitions.h:23-30).
 *     vrt_hip_last_error() gives the message of the last failure of a context.
 *   - the caller owns every host pointer; set_* calls copy; nothing is retained.
 *   - a context is bound to one device and is not thread-safe (the reference
 *     renders from one thread, main.cpp:257-296).
 *   - *_device variants take DEVICE pointers and a hipStream_t (as void*) and are
 *     asynchronous; the others take HOST pointers and return after completion.
 *   - Streams: frames enqueued through a *_device call run on the caller's stream and read
 *     the context's tables, lists and plane arrays.  Every call that rewrites one of those
 *     (set_gaussians*, set_plane, set_tiles, tile_gaussians with another tile size, a frame
 *     on another stream) first waits for the frames in flight, so no synchronisation by the
 *     caller is needed before changing state.  A stream passed to a *_device call has to
 *     stay valid until the context's next state change, vrt_hip_sync() or destroy.  The null
 *     stream (hip_stream == NULL: torch's default stream) is a stream like any other here:
 *     what was enqueued on it is waited for too, by the host-pointer forms as well, which
 *     run on the context's own non-blocking stream and share its buffers with the bundles.
 *
 * All paths are relative to /root/reference/src.
 */
#ifndef VRT_HIP_H
#define VRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vrt_hip_ctx vrt_hip_ctx;

typedef enum {
    VRT_HIP_OK = 0,
    VRT_HIP_ERR_INVALID = -1,   /* bad argument / call order            */
    VRT_HIP_ERR_HIP = -2,       /* a HIP runtime call failed             */
    VRT_HIP_ERR_NO_DEVICE = -3, /* no gfx950 device / no GPU             */
    VRT_HIP_ERR_NOMEM = -4
} vrt_hip_status;

/* Exp / Erf template arguments of the reference (rt.h:32,61,102,205,315,344;
 * defaults approx.h:110-127).  LIBM = expf/erff (rt.h:32 defaults), VCL = vcl_exp
 * (approx.h:91-106; ~1 ulp, flushes to 0 below -87.3), AS = Abramowitz-Stegun
 * (approx.cpp:90-110).  The others are the alternates of approx.cpp:9-188. */
enum { VRT_EXP_LIBM = 0, VRT_EXP_VCL = 1, VRT_EXP_FAST = 2, VRT_EXP_SPLINE = 3 };
enum { VRT_ERF_LIBM = 0, VRT_ERF_AS = 1, VRT_ERF_SPLINE = 2, VRT_ERF_SPLINE_MIRROR = 3, VRT_ERF_TAYLOR = 4 };

/* Pixel packing (rt.h:239-243 / 329-333 / 373-377): u32 = A<<24 | R<<16 | G<<8 | B. */
enum {
    VRT_PACK_TRUNC = 0,     /* (u32)(min(c,1)*255): scalar render_image, rt.h:240-242, 280-282        */
    VRT_PACK_ROUND = 1,     /* round-to-nearest-even (cvts): simd_render_image, rt.h:330-332, 374-376  */
    VRT_ALPHA_OPAQUE = 0,   /* A = 0xFF: rt.h:239, 279, 329                                           */
    VRT_ALPHA_COMPUTED = 2  /* A = round(min(1, sum albedo.w*inner)*255): tiled simd_render_image, rt.h:373 */
};

/* -------- context ---------------------------------------------------------------- */
/* Creates a context on HIP device `device`.  Fails with VRT_HIP_ERR_NO_DEVICE when no
 * GPU is visible -- there is no CPU fallback. */
int vrt_hip_create(int device, vrt_hip_ctx **out);
void vrt_hip_destroy(vrt_hip_ctx *ctx);
const char *vrt_hip_last_error(const vrt_hip_ctx *ctx); /* ctx may be NULL: last create() error */
const char *vrt_hip_version(void);

/* -------- scene: replaces gaussians_t / gaussian_vec_t (types.h:232-270) ----------- */
/* SoA upload == gaussian_vec_t::from_gaussians / load_gaussians (types.cpp:8-76).
 * albedo_a may be NULL (treated as 1, like simd_radiance rt.h:176).  n may be 0. */
int vrt_hip_set_gaussians(vrt_hip_ctx *ctx, size_t n, const float *mu_x, const float *mu_y, const float *mu_z,
                          const float *albedo_r, const float *albedo_g, const float *albedo_b,
                          const float *albedo_a, const float *sigma, const float *magnitude);
/* AoS upload == std::vector<gaussian_t> (types.h:195-200: albedo[4], mu[4], sigma, magnitude; 40 B). */
int vrt_hip_set_gaussians_aos(vrt_hip_ctx *ctx, size_t n, const void *gaussians);
/* The scene from DEVICE memory, for loops that keep their parameters on the GPU (an optimiser step, an animation): d_mu [n, 3],
 * d_albedo [n, 4] with alpha in column 3, d_sigma [n], d_magnitude [n], float32, packed -- the layout of a gradient bundle's columns.
 * The scene becomes exactly what vrt_hip_set_gaussians makes of the same values with albedo_a given: every later frame, query, bundle,
 * gradient row, statistic and the Morton index are the same bit for bit.  Everything is enqueued on `hip_stream` -- the read of the
 * caller's arrays, the scene tables, and the Morton index when vrt_hip_set_ray_index is on, which for such a scene is built by kernels
 * (also by the first bundle after it is switched on) -- and the call returns without waiting for it: the caller may overwrite its
 * arrays with later work on that stream.  Against work in flight the call is ordered like a bundle: on the stream of the last *_device
 * call nothing waits, a change of stream waits for the other stream.  Work on the context's own stream is ordered by events.
 * The two waits that remain:
 *   - a buffer that has to grow is freed first, which waits for the device: a larger n than before, the first call, more temporary
 *     storage for the index's sort.  With n unchanged no call waits;
 *   - the host keeps one value derived from the scene, the largest finite |albedo|, which scales the frame kernels' prune budget.  After
 *     a device update it is pending: the first frame afterwards (and vrt_hip_copy_state from this context) waits once for that update
 *     and reads one word back.  Bundles never need it: a loop of device updates and bundles never waits.
 * Host state changes as vrt_hip_set_gaussians changes it (caller-made tile lists are dropped, vrt_hip_state_generation advances by
 * one).  n == 0 is legal with NULL pointers; a NULL array with n > 0, or n > 0xFFFFFFF0, is VRT_HIP_ERR_INVALID and changes nothing. */
int vrt_hip_set_gaussians_device(vrt_hip_ctx *ctx, size_t n, const float *d_mu, const float *d_albedo, const float *d_sigma,
                                 const float *d_magnitude, void *hip_stream);

/* -------- tiling: replaces tile_gaussians + tiles_t (rt.cpp:29-69, types.h:272-287) - */
/* On-device binning with the reference's exact inclusion test, from the camera's view
 * matrix (column-major float[16], glm::mat4 layout).  tiles.w/h = ceil(2/tw), ceil(2/th). */
int vrt_hip_tile_gaussians(vrt_hip_ctx *ctx, float tw, float th, const float view[16]);
/* Same, asynchronous on `hip_stream` (no host synchronisation once tw/th have been seen before):
 * the per-frame form for animation loops (main.cpp:263 runs it every frame). */
int vrt_hip_tile_gaussians_device(vrt_hip_ctx *ctx, float tw, float th, const float view[16], void *hip_stream);
/* Caller-made tile sets as index lists into the uploaded scene: tile t (row-major,
 * tidx = ty*tiles_w + tx, rt.cpp:47-51) holds indices[offsets[t] .. offsets[t+1]). */
int vrt_hip_set_tiles(vrt_hip_ctx *ctx, float tw, float th, uint64_t tiles_w, uint64_t tiles_h,
                      const uint32_t *offsets, const uint32_t *indices);
/* Untiled rendering (the gaussians_t overloads, rt.h:227-228, 315-316): every ray sees every Gaussian. */
int vrt_hip_clear_tiles(vrt_hip_ctx *ctx);
/* Copies the current per-tile counts (tiles_w*tiles_h entries) to the host; for tests/statistics. */
int vrt_hip_get_tile_counts(vrt_hip_ctx *ctx, uint32_t *counts, size_t cap, uint64_t *tiles_w, uint64_t *tiles_h);
/* Copies tile t's index list (ascending scene order, like rt.cpp:52-62) to the host. */
int vrt_hip_get_tile_indices(vrt_hip_ctx *ctx, uint64_t t, uint32_t *indices, size_t cap, uint32_t *count);

/* -------- rays: replaces camera_t::projection_plane (camera.h:28-33, camera.cpp:50-71) */
/* Reference-style ray source: three w*h arrays of world-space plane points; ray i has
 * direction normalize(plane[i] - origin) (rt.h:231-237, 321-326, 366-371). */
int vrt_hip_set_plane(vrt_hip_ctx *ctx, uint32_t w, uint32_t h, const float *xs, const float *ys, const float *zs);
/* In-kernel ray generation from the camera basis: plane(i,j) = pos + x*right + y*up - focal*front,
 * x = -1 + j/(w/2), y = -1 + i/(h/2) -- the closed form of camera.cpp:52,60-69 (no 12 B/ray read). */
int vrt_hip_set_camera(vrt_hip_ctx *ctx, uint32_t w, uint32_t h, const float pos[3], const float right[3],
                       const float up[3], const float front[3], float focal);
/* In-kernel rays, bit for bit the reference's: the projection-plane point of pixel (i, j) is
 * inverse(view) * (-1 + j/(w/2), -1 + i/(h/2), 0, 1) (camera.cpp:60-69), evaluated per ray with glm's inverse and
 * glm's mat4*vec4 in their order of operations.  `view` = camera_t::view (column-major, glm layout).  Same image as
 * vrt_hip_set_plane() with the arrays camera_t would build, without the 12 B per ray.  (vrt_hip_set_camera above
 * takes the closed form pos + x right + y up - focal front instead: the same rays up to the rounding of the plane
 * points -- which the reference's |oc|^2 - mubar^2 can amplify to 1e-4 for small sigma.) */
int vrt_hip_set_camera_view(vrt_hip_ctx *ctx, uint32_t width, uint32_t height, const float view[16]);

/* width * height of the current ray set-up (0 before any set_plane / set_camera*). */
size_t vrt_hip_image_pixels(const vrt_hip_ctx *ctx);

/* -------- host camera: replaces camera_t (camera.h:20-44, camera.cpp:7-71) -------------------------------- */
/* Pure host code (no GPU needed, no context): the reference's yaw/pitch camera evaluated in glm's order of operations
 * (lookAtRH -> translate -> inverse -> mat4*vec4, unfused), so that view matrices and projection-plane points are the
 * reference's to the last bit whatever floating-point flags the CALLER is compiled with (csrc/vrt_host_camera.cpp).
 * Field meaning as in camera_t; `view` is camera_t::view_matrix, column-major (glm::mat4 layout). */
typedef struct {
    float position[3], front[3], up[3], world_up[3], right[3];
    float view[16];
    float focal_length;
    uint64_t w, h;
} vrt_hip_camera;
/* camera_t::camera_t (camera.cpp:25-36): stores the arguments, then turn(yaw, pitch). */
void vrt_hip_camera_init(vrt_hip_camera *cam, const float position[3], const float up[3], const float front[3],
                         float yaw, float pitch, uint64_t w, uint64_t h, float focal_length);
/* camera_t::turn (camera.cpp:7-23) + the view-matrix half of update() (camera.cpp:52); position is read as it is. */
void vrt_hip_camera_turn(vrt_hip_camera *cam, float yaw, float pitch, int constrain);
/* The view-matrix half of camera_t::update() alone (camera.cpp:52), from position / front / up / focal_length as stored. */
void vrt_hip_camera_refresh(vrt_hip_camera *cam);
/* The projection-plane half of camera_t::update() (camera.cpp:54-70): three w*h arrays, caller-allocated. */
void vrt_hip_camera_plane(const vrt_hip_camera *cam, float *xs, float *ys, float *zs);
/* The orbit step of the frame loop (main.cpp:252, 330): position = rotate(I, radians(deg), +Y) * (position, 1).
 * The caller follows it with `angle -= deg; turn(angle, 0)` like main.cpp:254-255, 332-333. */
void vrt_hip_camera_orbit(vrt_hip_camera *cam, float deg);
/* glm::inverse(mat4) in glm's order of operations (what camera.cpp:62 applies to view_matrix). */
void vrt_hip_mat4_inverse(const float m[16], float out[16]);

/* -------- options ---------------------------------------------------------------------- */
/* exp_kind / erf_kind: the reference's template arguments.  cull_eps: Gaussians whose
 * sigma*magnitude*exp(-d^2/(2 sigma^2)) is below cull_eps for every ray of an 8x8 pixel
 * block are skipped for that block (0 disables culling and reproduces the reference's
 * full O(5 N^2) sum).  Defaults: VRT_EXP_VCL, VRT_ERF_AS, cull_eps = 1e-9. */
int vrt_hip_set_options(vrt_hip_ctx *ctx, int exp_kind, int erf_kind, float cull_eps);
/* Mirror contexts (one frame needs one context: a batch of n frames needs n of them with the same scene): copies scene,
 * Exp / Erf / cull options, table settings and shard from src to dst (same device; device-to-device copies).  Rays, tiles
 * and statistics settings are not copied.  vrt_hip_state_generation() changes whenever one of the copied things changes. */
int vrt_hip_copy_state(vrt_hip_ctx *dst, const vrt_hip_ctx *src);
uint64_t vrt_hip_state_generation(const vrt_hip_ctx *ctx);
/* Image size of the rays last set (VRT_HIP_ERR_INVALID before vrt_hip_set_plane / set_camera / set_camera_view). */
int vrt_hip_get_image_size(const vrt_hip_ctx *ctx, uint32_t *w, uint32_t *h);

/* -------- render: replaces render_image / simd_render_image (rt.h:227-404) ------------- */
/* Renders the current scene/tiles/rays.  image_out: w*h u32 (nullable); radiance_out:
 * w*h*4 f32 = broadcast_radiance's vec4 per pixel before clamping (nullable).
 * Returns 0 when finished (the reference returns false = "not aborted"). */
int vrt_hip_render(vrt_hip_ctx *ctx, const float origin[3], int pack_flags, uint32_t *image_out, float *radiance_out);
int vrt_hip_render_device(vrt_hip_ctx *ctx, const float origin[3], int pack_flags, uint32_t *d_image,
                          float *d_radiance, void *hip_stream);

/* One animation frame in one call == the body of the reference's frame loop (main.cpp:259-296): tile_gaussians(view)
 * then render into d_image (raster order) or, when `shard` is non-zero, into this rank's compact shard buffer. */
int vrt_hip_frame_device(vrt_hip_ctx *ctx, float tw, float th, const float view[16], const float origin[3],
                         int pack_flags, uint32_t *d_out, int shard, void *hip_stream);
/* The same for a frame buffer that the CALLER promises still holds this context's previous frame, written by nothing else in
 * between (the reference's `image` is such a buffer: allocated once, written every frame, main.cpp:245): only the cells
 * that were lit in that frame and are empty now are reset to background, not all of them (16 MB of a 2048^2 frame's
 * 18.7 MB of HBM traffic).  The same frame, bit for bit.  One history per context: another buffer, image size, tile grid
 * or background value falls back to the full clear by itself; so does vrt_hip_frame (the library's own buffer gets this
 * treatment without being asked). */
int vrt_hip_frame_retained_device(vrt_hip_ctx *ctx, float tw, float th, const float view[16], const float origin[3],
                                  int pack_flags, uint32_t *d_out, void *hip_stream);

/* The same for callers without device memory of their own (the CLI): the frame goes to the context's own image
 * buffer on the context's stream.  image_out != NULL: copied out and waited for (a frame whose PNG is written);
 * image_out == NULL && !wait: returns as soon as the frame is enqueued -- an animation that only reports its
 * average frame time (main.cpp:310-315) keeps the GPU busy back to back; vrt_hip_sync() waits for the stream. */
int vrt_hip_frame(vrt_hip_ctx *ctx, float tw, float th, const float view[16], const float origin[3], int pack_flags,
                  uint32_t *image_out, int wait);
int vrt_hip_sync(vrt_hip_ctx *ctx);

/* -------- host frames: the frame loop's `image` in host memory (main.cpp:245, rt.h:344-346, 388-399) ---------------------
 * The reference renders every frame into a u32 *image that its caller allocated once in host memory (64-byte aligned,
 * main.cpp:245) and that the renderer overwrites frame after frame (rt.h:344-346, copy loop rt.h:388-399).  Register such
 * a buffer once; then each vrt_hip_frame_host enqueues the frame and its delivery into the buffer on the context's stream
 * and returns, and vrt_hip_sync waits.  A delivery writes only the 32x32-pixel cells that changed in that buffer since its
 * last delivery (cells lit now, and cells lit then that are dark now); the first delivery, another image size, tile grid or
 * background, and frames whose per-cell stamps were not kept (VRT_HIP_RETAIN_FRAME=0, a tile of more than 64 cells, a sharded
 * context) copy the whole frame: its w*h pixels, nothing beyond them in a larger buffer.  A frame without stamps records
 * nothing, so the delivery after it is a whole copy too.  A repeated pose is an ordinary frame: its lists are built anew, its
 * stamps kept, its delivery writes the lit cells again.  Dense frames: a buffer whose deliveries counted more than 3/4 of the
 * frame's cells (cells lit, or lit before and dark now) gets whole copies until they count less; the count a delivery reads
 * is that of the delivery before the previous one into that buffer (older while frames are in flight), so the switch lags by
 * two deliveries either way -- speed only, the pixels are the same.  Up to 16 buffers per context (a ring of frames in
 * flight), each with its own history and count. */
/* Page-locks and maps a caller-owned host buffer of `pixels` u32s for this context (hipHostRegister, mapped).  `image` must
 * be 64-byte aligned (what simd::aligned_malloc gives, main.cpp:245).  Refused (VRT_HIP_ERR_INVALID): NULL or misaligned
 * pointer, 0 pixels, a buffer already registered, with this or any context.  The buffer's history starts empty: its
 * next delivery is a full one. */
int vrt_hip_host_register(vrt_hip_ctx *ctx, uint32_t *image, size_t pixels);
/* Waits for every frame of this context still in flight, then unregisters the buffer.  vrt_hip_destroy does the same for
 * every buffer still registered. */
int vrt_hip_host_unregister(vrt_hip_ctx *ctx, uint32_t *image);
/* The frame of vrt_hip_frame (tile_gaussians + render into the context's own buffer, the same bits), then delivered into the
 * registered buffer `image` on the context's stream; returns once both are enqueued.  `image` holds the frame (its first
 * w*h pixels, what vrt_hip_frame(.., image_out, 1) returns) when vrt_hip_sync(ctx) returns.  The caller promises that
 * nothing but this context's deliveries wrote `image` since it was registered.  VRT_HIP_ERR_INVALID, with nothing
 * enqueued, when `image` is not registered with this context or holds fewer than w*h pixels. */
int vrt_hip_frame_host(vrt_hip_ctx *ctx, float tw, float th, const float view[16], const float origin[3], int pack_flags,
                       uint32_t *image);

/* Multi-GPU tile sharding: the context renders only tiles t with shard_of(t) == rank.
 * Owned tiles are written tile-major into a compact buffer of
 * vrt_hip_shard_pixels() u32s: [local tile][tile_h][tile_w].  assemble() scatters the
 * rank-major concatenation of all shards (e.g. an RCCL gather result) into raster order. */
int vrt_hip_set_shard(vrt_hip_ctx *ctx, int rank, int world);
size_t vrt_hip_shard_pixels(const vrt_hip_ctx *ctx);
int vrt_hip_render_shard_device(vrt_hip_ctx *ctx, const float origin[3], int pack_flags, uint32_t *d_shard,
                                void *hip_stream);
int vrt_hip_assemble_shards_device(vrt_hip_ctx *ctx, const uint32_t *d_gathered, uint32_t *d_image, void *hip_stream);
/* Same, for gathers that carry several frames per rank ([rank][frame][shard]): rank r's shard of the frame to
 * assemble starts at d_gathered + r * rank_stride_px (pass d_gathered already offset to the frame). */
int vrt_hip_assemble_shards_strided_device(vrt_hip_ctx *ctx, const uint32_t *d_gathered, size_t rank_stride_px,
                                           uint32_t *d_image, void *hip_stream);

/* Sparse shards: the transport format for small frames.  Most of a frame is background (95 % of `-g 64 -w 2048`), so a
 * rank ships only the 32x32-pixel cells that some Gaussian reaches.  Buffer layout, u32 words (16-byte aligned):
 *   [0] cells stored   [1] capacity C (cells)   [2] cells per tile   [3] 0
 *   [4 .. 4+C)         key of the cell in each slot: tile id * cells per tile + cell in tile (row-major 32-px cells)
 *   [P ..)             32*32 pixels per stored cell, P = 4 + C rounded up to a multiple of 4
 * C is the same on every rank of a job, so a fixed-size prefix [0, P + 1024 * max cells) can travel through a gather.
 * frame_sparse == vrt_hip_frame_device into such a buffer; scatter_sparse builds the raster frame on the assembling
 * rank: background everywhere, then every stored cell of every shard.  The shard pointers must be readable from this
 * context's device: own memory, a gathered copy, or another GPU's memory with peer access enabled (xGMI). */
/* words of a shard buffer for the CURRENT tile grid and shard (call after tile_gaussians / set_tiles / set_shard) */
size_t vrt_hip_sparse_shard_words(const vrt_hip_ctx *ctx);
int vrt_hip_frame_sparse_device(vrt_hip_ctx *ctx, float tw, float th, const float view[16], const float origin[3],
                                int pack_flags, uint32_t *d_sparse, void *hip_stream);
int vrt_hip_scatter_sparse_device(vrt_hip_ctx *ctx, const uint32_t *const *d_shards, int nshards, int pack_flags,
                                  uint32_t *d_image, void *hip_stream);
/* The same for a frame buffer that is reused frame after frame (the `image` of main.cpp:245, written every frame of the
 * loop): by calling this variant the caller promises that d_image still holds what the previous call of this variant on
 * this context left in it.  Then only the cells stored last time and not stored now are reset to background, instead
 * of all w * h pixels (16.8 MB per 2048^2 frame) -- the same frame, bit for bit.  A new buffer, image size, tile grid
 * or background falls back to the full fill by itself. */
int vrt_hip_scatter_sparse_retained_device(vrt_hip_ctx *ctx, const uint32_t *const *d_shards, int nshards, int pack_flags,
                                           uint32_t *d_image, void *hip_stream);
/* Several frames per assembly (the other end of vrt_hip_frame_batch_device): frame f is assembled into d_images[f] -- all
 * different buffers -- from shard s at d_shards[s] + f * frame_stride_words (what a gather of [rank][frame][prefix]
 * delivers), with one launch for all frames; retained != 0 as in the retained variant, per buffer (the context keeps a
 * history for up to 64 frame buffers; a call never drops the history of one of its own buffers to make room).
 * Caller contract, for all three scatter calls:
 *   - every shard starts on a 16-byte boundary (the pixels are read 16 bytes per lane), so frame_stride_words is a
 *     multiple of 4;
 *   - a shard whose header is not this job's ([1] != capacity or [2] != cells per tile), slots at and beyond [0], slots
 *     beyond the capacity and keys whose tile is beyond the grid are ignored, whatever they hold;
 *   - frame_stride_words may be a prefix P + 1024 k of the shard: slots at and beyond k are then not read, so a prefix
 *     must hold every stored cell (k >= [0] of every shard of every frame) -- except that the caller who finds a fuller
 *     shard afterwards gathers again and assembles again: the first assembly dropped the cells that did not travel;
 *   - a stride of exactly P words (the header alone) keeps ALL slots: it is only valid when [0] == 0 in every shard of
 *     every frame, slots below [0] would be read behind the prefix.
 * A rejected call (VRT_HIP_ERR_INVALID: 0 or more than 64 frames, more than 64 shards, a stride that is no multiple of
 * 4, two frames into one buffer, a tile size of 0 pixels) enqueues nothing and touches no frame buffer or history. */
int vrt_hip_scatter_sparse_batch_device(vrt_hip_ctx *ctx, const uint32_t *const *d_shards, int nshards,
                                        size_t frame_stride_words, int nframes, int pack_flags, uint32_t *const *d_images,
                                        int retained, void *hip_stream);

/* Several frames per launch: the animation loop of main.cpp:257-335 (`--frames N`: the orbit's cameras are known in advance)
 * with n frames handed over at once.  Frame i is rendered by ctxs[i] -- every frame needs a context of its own (lists,
 * queues and per-origin tables are per frame; same scene, options, rays' image size, tile grid and shard in all of them) --
 * with view matrix views[16 i ..] and origin origins[3 i ..] into d_out[i], exactly as vrt_hip_frame_device (out_kind 0),
 * vrt_hip_frame_device(.., shard = 1) (out_kind 1) or vrt_hip_frame_sparse_device (out_kind 2) would, bit for bit; but
 * each of the three kernels of a frame is launched ONCE for all n frames (grid.y = frame).  A sparse frame is tens of
 * microseconds of dependent launches: a batch pays the launch gaps and the kernels' tails once, and a rank that owns an
 * eighth of the tiles still fills its GPU.  Everything is enqueued on hip_stream; errors are reported through ctxs[0].
 * Not batched (VRT_HIP_ERR_INVALID): tiles of more than 64 cells, plane arrays that are no pinhole bundle. */
int vrt_hip_frame_batch_device(vrt_hip_ctx *const *ctxs, int n, float tw, float th, const float *views,
                               const float *origins, int pack_flags, uint32_t *const *d_out, int out_kind,
                               void *hip_stream);

/* -------- several GPUs from one process: replaces the thread pool over tiles (rt.h:355-399) one level up -------------
 * A group holds one context per entry of `devices` (a device may be listed more than once: each entry is a member
 * with its own stream -- how the protocol is tested on a one-GPU box).  Scene, options and rays are set per member
 * through vrt_hip_group_ctx(); vrt_hip_group_frame renders ONE frame tile-sharded over the members: member i renders
 * the tiles of shard (i, n) as a sparse shard on its own device and stream, member 0 waits for all of them (events),
 * reads the shards -- directly over xGMI where peer access exists, through a copy otherwise -- and assembles the
 * raster frame (the copy loop of rt.h:388-399).  Animations that do not need every frame in one place should deal
 * whole frames to the members instead (vrt_hip_frame on vrt_hip_group_ctx(g, k % n)): no exchange at all. */
typedef struct vrt_hip_group vrt_hip_group;
int vrt_hip_group_create(const int *devices, int n, vrt_hip_group **out);
void vrt_hip_group_destroy(vrt_hip_group *g);
int vrt_hip_group_size(const vrt_hip_group *g);
vrt_hip_ctx *vrt_hip_group_ctx(vrt_hip_group *g, int member);
const char *vrt_hip_group_last_error(const vrt_hip_group *g);
/* image_out (host, w*h u32) may be NULL; wait != 0 or image_out != NULL: returns when the frame is complete. */
int vrt_hip_group_frame(vrt_hip_group *g, float tw, float th, const float view[16], const float origin[3], int pack_flags,
                        uint32_t *image_out, int wait);
/* The assembled frame on member 0's device (valid until the next group_frame), for callers that keep it on the GPU. */
const uint32_t *vrt_hip_group_image_device(const vrt_hip_group *g);
int vrt_hip_group_sync(vrt_hip_group *g);
/* n frames of an animation tile-sharded over the members with ONE launch of each kernel per member and ONE assembly launch
 * on member 0 (vrt_hip_frame_batch_device + vrt_hip_scatter_sparse_batch_device): the frame loop of main.cpp:257-335 with
 * the orbit's next n cameras handed over at once.  A member's shard of a sparse frame is a few microseconds of work behind
 * three dependent launches: frame by frame the group is launch-bound and slower than one GPU; in batches the launches are
 * paid once per n frames.  views: 16 n floats, origins: 3 n floats; every frame is rendered with in-kernel rays of its view
 * matrix at the image size of member 0's rays (vrt_hip_set_camera_view / set_plane must have been called once).  The group
 * keeps n - 1 mirror contexts per member (scene, options and table settings copied from the member's own context whenever
 * vrt_hip_state_generation() says they changed).  images_out: NULL, or n host pointers (each NULL or w*h u32); returns when
 * the frames are complete if wait != 0 or any image is wanted.  Each frame equals vrt_hip_group_frame's, bit for bit.
 * n <= 64. */
int vrt_hip_group_frame_batch(vrt_hip_group *g, int n, float tw, float th, const float *views, const float *origins,
                              int pack_flags, uint32_t *const *images_out, int wait);
/* Frame f of the last batch on member 0's device (valid until the next batch). */
const uint32_t *vrt_hip_group_batch_image_device(const vrt_hip_group *g, int f);

/* -------- point queries: replace transmittance / radiance (rt.h:32-54, 146-223) ----------- */
/* T_out[k] = transmittance<Exp,Erf>(o, n, s[k], all Gaussians of the scene), rt.h:32-54. */
int vrt_hip_transmittance(vrt_hip_ctx *ctx, const float o[3], const float n[3], const float *s, size_t ns,
                          float *T_out);
/* T_out[r] = broadcast_transmittance (rt.h:102-127): ray r has its own origin origins[3*r..], unit direction
 * dirs[3*r..] and sample point s[r]; all Gaussians of the scene. */
int vrt_hip_transmittance_rays(vrt_hip_ctx *ctx, size_t nrays, const float *origins, const float *dirs, const float *s,
                               float *T_out);
/* out[4*r..] = radiance / broadcast_radiance (rt.h:146-164, 205-223) for ray r with origin
 * origins[3*r..], unit direction dirs[3*r..], over all Gaussians of the scene (no tiling). */
int vrt_hip_radiance(vrt_hip_ctx *ctx, size_t nrays, const float *origins, const float *dirs, float *out);
/* -------- ray bundles: broadcast_radiance (rt.h:205-223) for ANY rays, as a fast path ------------------------------------
 * Radiance (and optionally packed pixels) of nrays caller-given rays through the scene, culled per ray like the image
 * kernels' last level.  origins: 3 floats per ray (origin_per_ray != 0) or 3 floats in all (== 0: one origin for the
 * whole bundle).  dirs: 3 floats per ray, unit length (the caller normalises, like broadcast_radiance's callers).
 * d_radiance: 4 floats per ray (nullable); d_image: one u32 per ray, packed with pack_flags (nullable).
 * Uses the scene and vrt_hip_set_options (every Exp / Erf pair, cull_eps); ignores tiles, the rays of set_plane /
 * set_camera*, shard, table settings and cull_prune: an untiled bundle sees every Gaussian, as in the gaussians_t overloads.
 * Cull rule: a ray drops Gaussian j iff x > cull_x_j, x = (|oc|^2 - mubar^2) / (2 sigma_j^2), cull_x_j = ln(sigma_j mag_j /
 * eps_eff), eps_eff = cull_eps * min(1, 4096 / N), clamped at the point where Exp gives exactly 0 (cull_eps = 0: a ray keeps
 * everything Exp does not flush to exactly 0).  This is one level, entered by the whole scene, with the tile level's
 * threshold: a ray then loses less than 3 * cull_eps * min(N, 4096) = 1.23e-5 of radiance at the defaults, for any N.
 * Rays with at most 32 kept Gaussians are shaded lane = ray in the reference's summation order; longer lists by one wave per
 * ray, which sums in another (fixed) order.  Which of the two shades a ray depends on that ray alone: a ray's result is a
 * function of (ray, scene, options), whatever else is in the bundle.
 * The _device form takes device pointers and follows the stream rules at the top of this header: everything is enqueued on
 * hip_stream, without host synchronisation and without allocation once a bundle of at least this size has been seen; the
 * call counts as a frame in flight.  nrays == 0 returns VRT_HIP_OK with nothing launched; NULL dirs or origins with
 * nrays > 0, or both outputs NULL: VRT_HIP_ERR_INVALID, nothing enqueued.  vrt_hip_radiance below stays the full sum. */
int vrt_hip_radiance_rays_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray,
                                 const float *d_dirs, float *d_radiance, uint32_t *d_image, int pack_flags,
                                 void *hip_stream);
int vrt_hip_radiance_rays(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                          float *radiance_out, uint32_t *image_out, int pack_flags);        /* host pointers, waits */
/* -------- transmittance bundles: broadcast_transmittance (rt.h:102-127) for ANY rays at ANY number of depths, as a fast path --
 * T[r * ns + k] = Exp(sum_j term_j(s[r, k])) over the Gaussians ray r keeps under the cull rule of the ray bundles above (the same
 * cull_x, the same eps_eff, the same code); term_j is the reference's term in the reference's operations and order (unfused, exact
 * divides), as in vrt_hip_transmittance_rays.  A ray that keeps nothing gets Exp(0) of the selected kind.
 * origins, origin_per_ray, dirs: as in vrt_hip_radiance_rays_device.  s: ns sample distances shared by all rays (s_per_ray == 0) or
 * nrays * ns of them, [r * ns + k] (s_per_ray != 0).  Any ns >= 1: the kernels loop.  s must be finite; a negative s is allowed
 * and gives T > 1, as the point query does.  Shadow rays are ns = 1; a depth profile of a ray is one call.
 * Cull bound: a dropped Gaussian has sigma mag exp(-x) < eps_eff, and its term is at most 2 / sqrt(2 pi) times that, so the
 * exponent moves by less than 0.8 * cull_eps * min(N, 4096) = 3.3e-6 at the defaults -- and for s >= 0, where T <= 1, T moves by
 * less than that.  cull_eps = 0 keeps everything that Exp does not flush to exactly 0.
 * Rays with at most 32 kept Gaussians are summed lane = ray in ascending scene order (the reference's sum without what the cull
 * dropped); longer lists by one wave per ray, which sums in another (fixed) order.  A result is a function of (ray, s, scene,
 * options) alone, whatever else is in the bundle and however many samples the call carries.
 * Uses the scene, every Exp / Erf pair, cull_eps and the Morton index when vrt_hip_set_ray_index is on (the same bits either way);
 * ignores tiles, the rays of set_plane / set_camera*, shard, table settings and cull_prune.
 * The rules are the radiance bundle's: everything is enqueued on hip_stream, without host synchronisation and without allocation
 * once a bundle of at least this size has been seen (nrays, and nrays * ns for s and T of the host form); the call counts as a
 * frame in flight.  It shares the context's long-ray queue, counters, scratch slots and bitmap with the radiance bundles: two
 * bundles of one context are ordered by the stream they share.  nrays == 0 or ns == 0 returns VRT_HIP_OK with nothing launched;
 * NULL dirs, origins, s or T with work to do, or more rays than the u32 queue holds: VRT_HIP_ERR_INVALID, nothing enqueued.
 * vrt_hip_get_ray_stats / vrt_hip_get_ray_index_stats report the last bundle of either kind; for the same rays, scene and options
 * every field is what a radiance bundle reports.  vrt_hip_transmittance_rays stays the full sum. */
int vrt_hip_transmittance_bundle_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray,
                                        const float *d_dirs, const float *d_s, size_t ns, int s_per_ray, float *d_T,
                                        void *hip_stream);
int vrt_hip_transmittance_bundle(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                                 const float *s, size_t ns, int s_per_ray, float *T_out);       /* host pointers, waits */
/* -------- depth bundles: the distance along ANY rays at which T falls to a level -- the inverse of the transmittance bundles ----
 * depth[r * nt + k] = where ray r's transmittance reaches the level tau[k] (tau_per_ray == 0: nt levels shared by all rays) or
 * tau[r * nt + k] (tau_per_ray != 0): a first-hit distance (tau = 0.5: the median depth), a depth map at any level for compositing,
 * the free-flight distance of a path tracer ("the s with T(s) = xi").  Any nt >= 1: the kernels loop.
 * That(r, s) is what vrt_hip_transmittance_bundle returns for ray r at distance s under the same scene and options: the same cull,
 * the same terms, the same summation order, the selected Exp and Erf -- bit for bit.  s_end(r) = max over the Gaussians the ray
 * keeps of mubar_j + 6 sqrt(2) sigma_j, at least 0: every Erf is saturated there.  With tau the level:
 *   tau is NaN                                        NaN
 *   That(r, 0) <= tau  (every tau >= 1: That(r, 0) = Exp(0))   0
 *   the ray keeps nothing, or That(r, s_end) > tau    +inf: the ray never gets that dark (every tau <= 0 that That does not reach)
 *   otherwise                                         the upper end hi of a bracket lo < hi with That(r, hi) <= tau < That(r, lo), both
 *                                                     ends evaluated by the kernel, narrowed by bisection from [0, s_end] until
 *                                                     hi - lo <= max(ulp(hi), s_end * 2^-24)
 * The comparison is made in T with the selected Exp (not in the exponent against ln tau): vrt_hip_transmittance_bundle at s = depth
 * on the same context returns a T <= tau, exactly.  With magnitudes >= 0 T does not increase along a ray and the crossing is
 * unique up to that resolution and the rounding of That; with negative magnitudes the result is still such a bracket, around one of
 * the crossings.  A result is a function of (ray, tau, scene, options) alone, whatever else is in the bundle, however many levels the
 * call carries and whether the Morton index is on.
 * Cost: per ray two walks of its list (s_end with That(0), That(s_end)), then one walk per halving -- 23 to 25 -- for every group of
 * up to 4 levels; the cull is paid once.
 * origins, origin_per_ray, dirs, the stream rules, the buffers that only grow (nrays, and nrays * nt for tau and depth of the host
 * form), the shared queue / counters / scratch slots / bitmap and the statistics are the transmittance bundle's: two bundles of one
 * context are ordered by the stream they share; vrt_hip_get_ray_stats / vrt_hip_get_ray_index_stats report the last bundle of any of
 * the three kinds, and for the same rays, scene and options every field is what a radiance bundle reports.  nrays == 0 or nt == 0
 * returns VRT_HIP_OK with nothing launched; NULL origins, dirs, tau or depth with work to do, more than 2^32 - 16 rays, or an
 * nrays * nt that does not fit: VRT_HIP_ERR_INVALID, nothing enqueued. */
int vrt_hip_depth_bundle_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                const float *d_tau, size_t nt, int tau_per_ray, float *d_depth, void *hip_stream);
int vrt_hip_depth_bundle(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                         const float *tau, size_t nt, int tau_per_ray, float *depth_out);           /* host pointers, waits */
/* -------- gradient bundles: d(loss) / d(Gaussians) from d(loss) / d(radiance) of ANY rays -------------------------------------
 * The function that is differentiated is what vrt_hip_radiance_rays computes for the same rays, scene and options:
 *   L(r) = sum_{i in K} a_i sum_{k=-4..0} sigma_i m_i exp(-d2_i / (2 sigma_i^2) - k^2 / 2) T(mubar_i + k sigma_i),
 *   T(s) = Exp(sum_{j in K} A_j (Erf(-mubar_j r_j) - Erf((s - mubar_j) r_j))),  A_j = sigma_j m_j exp(-d2_j / (2 sigma_j^2)) / 0.79788456,
 * with K the list ray r keeps under the cull rule of the ray bundles above (the same cull_x, the same eps_eff, the same code) HELD
 * FIXED: the cull is piecewise constant in the parameters, so a Gaussian that a ray drops gets nothing from that ray -- in
 * particular one of magnitude 0, which every ray drops.  Given grad_radiance[4 * r ..] = d(loss) / d(L(r)), row j of the table gets
 *   [0..3] d(loss) / d(albedo rgba of j)   [4..6] d / d(mu xyz)   [7] d / d(sigma)   [8] d / d(magnitude)   [9..11] never touched
 * summed over the rays that keep j.  Exp and Erf in L and T are the selected pair's; their derivatives are the analytic ones
 * (Exp' = Exp, Erf'(x) = 2 / sqrt(pi) exp(-x^2)), also for the Abramowitz-Stegun Erf.  Supported pairs: {vcl_exp, expf} x
 * {A&S erf, erff}; under any other pair the call returns VRT_HIP_ERR_INVALID with a message and enqueues nothing (the piecewise
 * approximations have jumps).  The gradient with respect to the rays themselves is the _rays form's, below.
 * The _device form ADDS into d_grad (N rows of VRT_HIP_GRAD_STRIDE floats, N = Gaussians of the scene) with float atomics: the
 * caller clears the table, and may let several bundles add into it.  A row of a Gaussian that no ray keeps is not written at all.
 * The sums depend on the arrival order of the atomic adds: results are NOT bitwise reproducible from run to run, unless
 * vrt_hip_set_grad_ordered (below) is on.  d_grad_radiance
 * is 16-byte aligned, as d_radiance of vrt_hip_radiance_rays_device.  The host form overwrites grad_out (columns 9..11 with 0).
 * Everything else is the radiance bundle's: origins, origin_per_ray, dirs, the stream rules, the buffers that only grow, the shared
 * queue / counters / scratch slots / bitmap, the Morton index (the same kept lists either way), "counts as a frame in flight";
 * vrt_hip_get_ray_stats / vrt_hip_get_ray_index_stats report for the same rays every field a radiance bundle reports, and the
 * same rays go to the same kind of kernel.  nrays == 0 or a scene of no Gaussians returns VRT_HIP_OK with nothing launched and the
 * table untouched; NULL origins, dirs, grad_radiance or table with work to do, more than 2^32 - 16 rays, or an unsupported pair:
 * VRT_HIP_ERR_INVALID, nothing enqueued. */
enum { VRT_HIP_GRAD_STRIDE = 12 };  /* floats per row: [0..3] d albedo rgba, [4..6] d mu xyz, [7] d sigma, [8] d magnitude, [9..11] never touched */
int vrt_hip_radiance_rays_grad_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                      const float *d_grad_radiance /* 4 per ray */, float *d_grad /* N rows, ACCUMULATED into */,
                                      void *hip_stream);
int vrt_hip_radiance_rays_grad(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                               const float *grad_radiance, float *grad_out /* N rows, OVERWRITTEN; columns 9..11 written as 0 */);
/* -------- transmittance gradient bundles: d(loss) / d(Gaussians, samples) from d(loss) / d(T) of ANY rays, and the same for depths ----
 * The function that is differentiated is what vrt_hip_transmittance_bundle computes for the same rays, samples, scene and options:
 *   T(r, k) = Exp(E_k),  E_k = sum_{j in K} A_j (Erf(-mubar_j r_j) - Erf((s_k - mubar_j) r_j)),  A_j = sigma_j m_j exp(-d2_j / (2 sigma_j^2)) / 0.79788456,
 * r_j = 1 / (sqrt2 sigma_j), with K the list ray r keeps under the cull rule of the ray bundles HELD FIXED, as in the gradient bundles
 * above (a Gaussian of magnitude 0 is dropped by every ray and gets nothing).  S_k = dE_k / ds_k, so that dT / ds = T S.
 * wrt == VRT_HIP_TGRAD_T: grad_T[r * ns + k] = d(loss) / d(T(r, k)).  Row j of the table gets, summed over the rays that keep j and
 *   their samples, [4..6] d(loss) / d(mu xyz of j), [7] d / d(sigma), [8] d / d(magnitude); grad_s[r * ns + k] = d(loss) / d(s[r, k]) =
 *   grad_T T S (with shared samples, s_per_ray == 0, the caller sums it over the rays).
 * wrt == VRT_HIP_TGRAD_DEPTH: s holds the depths vrt_hip_depth_bundle returned for levels tau (s_per_ray != 0, ns = nt), grad_T[r * ns
 *   + k] = d(loss) / d(depth[r, k]).  The table gets d(loss) / d(Gaussians) by the implicit function theorem on T(depth, Gaussians) =
 *   tau: every sample weighs -grad_T / S_k instead of grad_T T_k; grad_s[r * ns + k] = d(loss) / d(tau[r, k]) = grad_T / (T_k S_k).
 *   This is the derivative of the IDEAL crossing T(depth) = tau, not of the upper end of the bracket the depth bundle returns (the two
 *   differ by the bracket's width, which the derivative does not see).  A sample whose s is not finite or <= 0, or at which S_k == 0
 *   -- the depth bundle's +inf, 0 and NaN results -- contributes exactly nothing, and its grad_s is 0.
 * In both modes a sample with grad_T == 0 is skipped exactly, whatever its s (NaN included), and its grad_s is 0: a caller masks
 * samples with zeros.  Other values that are not finite propagate as the arithmetic makes them.
 * Columns 0..3 (albedo: T does not depend on it) and 9..11 of the table are never touched, nor the rows of Gaussians that no ray
 * keeps: one table may collect a radiance gradient and a mask or depth gradient.  The _device form ADDS into d_grad with float
 * atomics (not bitwise reproducible unless vrt_hip_set_grad_ordered, below, is on) and STORES d_grad_s; either may be NULL, not both.  The host form overwrites grad_out (N rows,
 * untouched entries 0) and grad_s_out.  Exp and Erf of the forward quantities are the selected pair's, the derivatives the analytic
 * ones; supported pairs as above: {vcl_exp, expf} x {A&S erf, erff}.  The gradient with respect to the rays is the _rays form's, below.
 * Everything else is the gradient bundle's contract: origins, origin_per_ray, dirs, the stream rules, the buffers that only grow, the
 * shared queue / counters / scratch slots / bitmap, the Morton index (the same kept lists either way), the statistics (for the same
 * rays every field a radiance bundle reports).  nrays == 0, ns == 0 or a scene of no Gaussians returns VRT_HIP_OK with nothing
 * launched and nothing written; NULL origins, dirs, s or grad_T with work to do, both outputs NULL, wrt outside {0, 1}, an
 * unsupported pair, more than 2^32 - 16 rays or an nrays * ns that does not fit: VRT_HIP_ERR_INVALID with a message, nothing enqueued. */
enum { VRT_HIP_TGRAD_T = 0, VRT_HIP_TGRAD_DEPTH = 1 };
int vrt_hip_transmittance_bundle_grad_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                             const float *d_s, size_t ns, int s_per_ray, const float *d_grad_T /* nrays * ns */, int wrt,
                                             float *d_grad /* N rows of VRT_HIP_GRAD_STRIDE, ADDED into; may be NULL */,
                                             float *d_grad_s /* nrays * ns, stored; may be NULL */, void *hip_stream);
int vrt_hip_transmittance_bundle_grad(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                                      const float *s, size_t ns, int s_per_ray, const float *grad_T, int wrt,
                                      float *grad_out /* N rows, OVERWRITTEN, or NULL */, float *grad_s_out /* nrays * ns, or NULL */);
/* -------- ray gradients: d(loss) / d(origin, direction) of every ray, from either gradient bundle -----------------------------------
 * The _rays forms are the two gradient bundles above with one more output: grad_rays, nrays rows of VRT_HIP_RAY_GRAD_STRIDE floats,
 *   [0..2] d(loss) / d(origin of ray r)   [3] 0   [4..6] the tangential d(loss) / d(dir of ray r)   [7] 0
 * of the same function under the same fixed kept lists.  Every observable depends on a ray (o, n) through c_j = mu_j - o and n alone;
 * with ray r's share of row j's d mu written as a_j c_perp_j + b_j n (c_perp_j = c_j - mubar_j n, mubar_j = c_j . n),
 *   d(loss) / d(o) = -sum_{j in K} (a_j c_perp_j + b_j n),      d(loss) / d(n) = sum_{j in K} (b_j - a_j mubar_j) c_perp_j.
 * The tangential derivative is defined so: for a unit t perpendicular to dir, (row[4..6] . t) = d/d(eps) of the loss along the rays
 * normalise(dir + eps t) at eps = 0.  The row is perpendicular to dir (to rounding): a caller who normalises a raw vector v gets
 * d(loss) / d(v) = row[4..6] / |v|, which torch's normalize does by itself.  With a shared origin (origin_per_ray == 0) the rows are
 * still per ray, and the caller sums columns 0..2 over the rays, as grad_s of shared samples.
 * The rows are STORED, never added: every ray r < nrays gets a row, a ray that keeps nothing one of exact zeros, and nothing behind
 * row nrays - 1 is written.  No atomic add takes part in them: a ray's row is summed in the order of its kept list (one wave per ray: in
 * the fixed order of the wave's lanes), so the ray rows ARE bitwise reproducible -- from run to run, with the Morton index on or off,
 * with or without the table, host or device form -- while the table is not, unless vrt_hip_set_grad_ordered (below) is on.
 * d_grad_rays is 16-byte aligned.
 * d_grad / grad_out may be NULL: then no atomic add is issued at all (a pose-only fit).  d_grad_rays / grad_rays_out may be NULL: then
 * the call is the form above without _rays.  At least one output must be non-NULL: VRT_HIP_ERR_INVALID with the bundle kind's message
 * otherwise.  In depth mode a sample that contributes nothing to the table contributes nothing to the ray's row.  Everything else --
 * the checks and their messages, a bundle of nothing (nothing launched, nothing written), the supported pairs, the stream rules, the
 * buffers that only grow, the statistics, the Morton index -- is the gradient bundle's contract. */
enum { VRT_HIP_RAY_GRAD_STRIDE = 8 };  /* floats per ray row: [0..2] d origin, [3] 0, [4..6] tangential d direction, [7] 0 */
int vrt_hip_radiance_rays_grad_rays_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                           const float *d_grad_radiance /* 4 per ray */, float *d_grad /* N rows, ADDED into; may be NULL */,
                                           float *d_grad_rays /* nrays rows of VRT_HIP_RAY_GRAD_STRIDE, STORED; may be NULL */, void *hip_stream);
int vrt_hip_radiance_rays_grad_rays(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                                    const float *grad_radiance, float *grad_out /* N rows, OVERWRITTEN, or NULL */,
                                    float *grad_rays_out /* nrays rows, or NULL */);
int vrt_hip_transmittance_bundle_grad_rays_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                                  const float *d_s, size_t ns, int s_per_ray, const float *d_grad_T /* nrays * ns */, int wrt,
                                                  float *d_grad /* ADDED into; may be NULL */, float *d_grad_s /* stored; may be NULL */,
                                                  float *d_grad_rays /* nrays rows of VRT_HIP_RAY_GRAD_STRIDE, STORED; may be NULL */, void *hip_stream);
int vrt_hip_transmittance_bundle_grad_rays(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                                           const float *s, size_t ns, int s_per_ray, const float *grad_T, int wrt,
                                           float *grad_out /* N rows, OVERWRITTEN, or NULL */, float *grad_s_out /* nrays * ns, or NULL */,
                                           float *grad_rays_out /* nrays rows, or NULL */);
/* -------- tangent bundles: J . v of the radiance of ANY rays, forward mode -----------------------------------------------------------
 * The other half of the gradient bundles: they give J^T . u, from d(loss) / d(radiance) to d(loss) / d(Gaussians, rays); this gives
 * J . v, how the radiance of every ray moves when the Gaussians and the rays move along a given direction v (a Gauss-Newton step by
 * conjugate gradients needs J^T (J v); a sensitivity image is J v for a one-hot v).  The function is the one the gradient bundles
 * differentiate (the formula at "gradient bundles" above): L(r) over the list K that ray r keeps under the bundles' cull rule, HELD
 * FIXED, Exp and Erf the selected pair's, their derivatives the analytic ones, also for the Abramowitz-Stegun Erf.  Supported pairs:
 * {vcl_exp, expf} x {A&S erf, erff}; under any other pair the call returns VRT_HIP_ERR_INVALID with a message and enqueues nothing.
 * The direction:
 *   tangent      N rows of VRT_HIP_GRAD_STRIDE floats, the gradient table's layout (J and J^T share one layout):
 *                [0..3] d albedo rgba   [4..6] d mu xyz   [7] d sigma   [8] d magnitude   [9..11] never read
 *   ray_tangent  nrays rows of VRT_HIP_RAY_GRAD_STRIDE floats, the ray rows' layout, per ray also when origin_per_ray == 0:
 *                [0..2] d origin   [3] never read   [4..6] d direction   [7] never read
 *                Of d direction only the part perpendicular to dir counts: the derivative is taken along normalise(dir + eps t).  (It
 *                enters through c_perp_j . t alone, which drops the part along dir to rounding, as the ray rows are perpendicular
 *                to dir to rounding: J . v is the transpose of the _rays forms' rows term for term.)
 * Either may be NULL, which means zero; both NULL: VRT_HIP_ERR_INVALID.  The result:
 *   out[4 r ..] = sum_{j in K(r)} dL(r) / d(theta_j) . tangent_j  +  dL(r) / d(o, n) . ray_tangent_r          4 floats per ray, STORED
 * A Gaussian that a ray drops contributes nothing to that ray, whatever its row holds (its row is not read for it) -- one of magnitude
 * 0 is such a case for every ray; a ray that keeps nothing gets zeros; nothing behind ray nrays - 1 is written.
 * With c = mu - o, mubar = c . n, c_perp = c - mubar n, d2 = |c_perp|^2, r = 1 / (sqrt2 sigma), C = 2 / sqrt(pi), dn the tangential part
 * of the ray's direction tangent, x_ikj = (mubar_i + k sigma_i - mubar_j) r_j, D_ikj = Erf(-mubar_j r_j) - Erf(x_ikj), e1_j =
 * exp(-(mubar_j r_j)^2), e2_ikj = exp(-x_ikj^2) and t_ik the ik term of L without its albedo, the chain rule gives
 *   dc_j = dmu_j - do,   dmubar_j = dc_j . n + c_perp_j . dn,   dd2_j = 2 c_perp_j . dc_j - 2 mubar_j (c_perp_j . dn),
 *   dA_j = A_j (dsigma_j / sigma_j - dd2_j / (2 sigma_j^2) + d2_j dsigma_j / sigma_j^3) + (A_j / m_j) dm_j        (A_j / m_j formed without dividing)
 *   dx_ikj = (dmubar_i + k dsigma_i - dmubar_j) r_j - x_ikj dsigma_j / sigma_j,
 *   dD_ikj = C [e1_j (-dmubar_j r_j + mubar_j r_j dsigma_j / sigma_j) - e2_ikj dx_ikj],     dE_ik = sum_j (dA_j D_ikj + A_j dD_ikj),
 *   dL = sum_ik [da_i t_ik + a_i t_ik (dsigma_i / sigma_i + dm_i / m_i - dd2_i / (2 sigma_i^2) + d2_i dsigma_i / sigma_i^3 + dE_ik)]   (no division by m_i either)
 * ONE pass over the (emitter, sample, absorber) pairs; every result is a store; no atomic add takes part and there is no table, so a
 * result is a function of (ray, its ray tangent, the tangent rows of the Gaussians it keeps, scene, options) alone: bitwise
 * reproducible from run to run, host or device form, whatever the other rays of the bundle are, with vrt_hip_set_ray_index and
 * vrt_hip_set_ray_sort on or off (the same bits at the same ray index).  vrt_hip_set_grad_ordered has no effect here.
 * d_tangent, d_ray_tangent and d_out are 16-byte aligned.  Everything else is the gradient bundle's contract: origins, origin_per_ray,
 * dirs, the stream rules (everything enqueued on hip_stream, no host wait, no allocation once a bundle of this size has been seen), the
 * buffers that only grow, the shared queue / counters / scratch slots / bitmap, "counts as a frame in flight";
 * vrt_hip_get_ray_stats / vrt_hip_get_ray_index_stats report for the same rays every field a radiance bundle reports, and the same rays
 * go to the same kind of kernel.  nrays == 0 or a scene of no Gaussians returns VRT_HIP_OK with nothing launched and nothing written;
 * NULL origins, dirs or out with work to do, both inputs NULL, more than 2^32 - 16 rays, or an unsupported pair: VRT_HIP_ERR_INVALID
 * with a message, nothing enqueued.  The host form stages tangent, ray_tangent and out in context buffers that only grow and waits once. */
int vrt_hip_radiance_rays_tangent_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                         const float *d_tangent      /* N rows of VRT_HIP_GRAD_STRIDE, or NULL */,
                                         const float *d_ray_tangent  /* nrays rows of VRT_HIP_RAY_GRAD_STRIDE, or NULL */,
                                         float *d_out                /* 4 per ray, STORED */, void *hip_stream);
int vrt_hip_radiance_rays_tangent(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                                  const float *tangent, const float *ray_tangent, float *out);   /* host pointers, waits */
/* -------- Gauss-Newton diagonal bundles: diag(J^T W J) of the radiance of ANY rays ---------------------------------------------------
 * The third part of a Gauss-Newton or Levenberg-Marquardt fit next to J^T u (the gradient bundles) and J . v (the tangent bundles): for
 * every parameter theta of every Gaussian (albedo rgba, mu xyz, sigma, magnitude)
 *   D[theta] = sum_r sum_{c=0..3} w[r, c] (d L_c(r) / d theta)^2
 * -- the Jacobi preconditioner of a CG solve on J^T W J, Marquardt's damping J^T W J + lambda diag(J^T W J), and the per-parameter
 * sensitivity of the rays.  L, the kept list K held fixed, the cull, the analytic derivatives and the supported pairs are exactly those
 * stated for vrt_hip_radiance_rays_grad above: the row of channel c is that bundle's row for grad_radiance = e_c, and the rows are
 * squared PER RAY AND CHANNEL before anything is summed.  Row j of the table has the gradient table's layout:
 *   [0..3] D of albedo rgba of j   [4..6] D of mu xyz   [7] D of sigma   [8] D of magnitude   [9..11] never touched
 * and the albedo columns are sum_r w[r, c] (m_j V_j)^2, since d L_c / d a_jc' = delta_cc' m_j V_j.  weights: 4 floats per ray, 16-byte
 * aligned in the device form, or NULL for all 1; they are not required to be non-negative (the sum is linear in them); under
 * non-negative weights every entry is >= 0.
 * The _device form ADDS into d_diag (N rows of VRT_HIP_GRAD_STRIDE floats) with float atomics: the caller clears the table, and may let
 * several bundles add into it.  A row of a Gaussian that no ray keeps is not written at all; a Gaussian of magnitude 0, which every ray
 * drops, gets nothing.  Not bitwise reproducible from run to run -- unless vrt_hip_set_grad_ordered is on: then every (ray, kept
 * Gaussian) files ONE record (long rays too), the ray's own share of D, the table gets the ordered sums with the bits that contract
 * states (segment depth ceil(n_j / 64) + 6 for n_j rays that keep j), and vrt_hip_get_grad_records returns the shares.  The host form
 * overwrites diag_out (columns 9..11 with 0).
 * Everything else is the gradient bundle's contract: origins, origin_per_ray, dirs, the stream rules, the buffers that only grow, the
 * shared queue / counters / scratch slots / bitmap, the Morton index, vrt_hip_set_ray_sort and a bound ray plan (the same kept lists
 * either way), "counts as a frame in flight"; vrt_hip_get_ray_stats / vrt_hip_get_ray_index_stats report for the same rays every field a
 * radiance bundle reports, and the same rays go to the same kind of kernel.  One buffer more belongs to the context and only grows: a
 * ray whose list is longer than 1024 keeps 48 bytes per further list position in a workspace of (N - 1024) * 48 bytes per workgroup of
 * the one-wave-per-ray kernel, 256 MB in all at the most where more than one workgroup runs (fewer workgroups for larger scenes); the
 * kernel never runs on fewer than one workgroup, whose single slot passes 256 MB from N = 5.6 M on and is reserved in full.
 * nrays == 0 or a scene of no Gaussians returns VRT_HIP_OK with nothing launched and the table untouched; NULL origins, dirs or table
 * with work to do, more than 2^32 - 16 rays, or an unsupported pair: VRT_HIP_ERR_INVALID with a message, nothing enqueued. */
int vrt_hip_radiance_rays_gn_diag_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                         const float *d_weights /* 4 per ray, or NULL = all 1 */,
                                         float *d_diag /* N rows of VRT_HIP_GRAD_STRIDE, ADDED into */, void *hip_stream);
int vrt_hip_radiance_rays_gn_diag(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                                  const float *weights, float *diag_out /* N rows, OVERWRITTEN; columns 9..11 written as 0 */);
/* -------- transmittance tangent bundles: J . v of the transmittance and of the depth of ANY rays, forward mode -----------------------
 * The other half of the transmittance gradient bundles, as the tangent bundles are of the gradient bundles: they give J^T . u in T and
 * in depth mode, this gives J . v -- how T(r, s_k), or the depth at which T falls to a level, moves when the Gaussians, the rays and
 * the samples (or levels) move along a given direction.  With it every observable of the ray bundles has value, J^T u and J v: a
 * Gauss-Newton step on a loss with mask, shadow-ray or depth terms has its J^T (J v), and a sensitivity image of a depth map is ONE call.
 * The function, the kept list K(r) HELD FIXED, the notation (A_j, r_j, m_j, C, x_kj, D_kj, e1_j, e2_kj, E_k, T_k, S_k) and the supported
 * pairs are those of "transmittance gradient bundles" above.  The direction, every part nullable (NULL means zero; all three NULL:
 * VRT_HIP_ERR_INVALID):
 *   tangent      N rows of VRT_HIP_GRAD_STRIDE floats, the gradient table's layout: [4..6] d mu xyz, [7] d sigma, [8] d magnitude;
 *                columns 0..3 (T does not depend on the albedo) and 9..11 are never read
 *   ray_tangent  nrays rows of VRT_HIP_RAY_GRAD_STRIDE floats, the tangent bundles' (only the part of d direction perpendicular to
 *                dir counts; [3] and [7] never read)
 *   s_tangent    d s[r, k] (wrt == VRT_HIP_TGRAD_T) or d tau[r, k] (VRT_HIP_TGRAD_DEPTH): nrays * ns floats [r * ns + k], or ns shared
 *                by the rays when s_tangent_per_ray == 0 (independent of s_per_ray)
 * From the tangent bundles' three scalars per (ray, kept Gaussian) -- dmubar_j, ds_j = dsigma_j / sigma_j and dA_j (their formulas
 * above, with the same dc_j = dmu_j - do and c_perp_j . dn):
 *   dE_k = sum_j [ dA_j D_kj + A_j C e2_kj (dmubar_j r_j + x_kj ds_j) ] + sum_j A_j C e1_j (m_j ds_j - dmubar_j r_j)
 *   wrt == VRT_HIP_TGRAD_T:      out[r * ns + k] = T_k (dE_k + S_k ds_k)                        at the samples s
 *   wrt == VRT_HIP_TGRAD_DEPTH:  out[r * ns + k] = (dtau_k / T_k - dE_k) / S_k                  at s = the depths a depth bundle returned
 * Depth mode is the implicit function theorem on T(depth, theta) = tau, the derivative of the IDEAL crossing, as in the gradient
 * bundles, and takes s_per_ray != 0 (s_per_ray == 0: VRT_HIP_ERR_INVALID).  There a sample whose s_k is not finite or <= 0, or whose
 * S_k == 0 (the depth bundle's +inf, 0 and NaN results) gets exactly 0.  In T mode values that are not finite propagate as the
 * arithmetic makes them.  This is the transpose, term for term, of vrt_hip_transmittance_bundle_grad_rays (table columns 4..8, ray rows,
 * grad_s): sum_rk g[r, k] out[r, k] = <table, tangent> + <ray rows, ray_tangent> + <grad_s, s_tangent> to rounding.
 * ONE walk of a ray's list per group of samples (the gradient bundles make two); every result is a STORE, no atomic add and no table:
 * a result is a function of (ray, its samples, its part of the direction, the tangent rows of the Gaussians it keeps, scene, options)
 * alone, bitwise reproducible from run to run, host or device form, whatever the other rays of the bundle are, with
 * vrt_hip_set_ray_index and vrt_hip_set_ray_sort on or off (the same bits at the same ray index); vrt_hip_set_grad_ordered has no effect.
 * A Gaussian that a ray drops contributes nothing to that ray (its row is not read for it); a ray that keeps nothing gets zeros; nothing
 * behind out[nrays * ns - 1] is written.
 * d_tangent and d_ray_tangent are 16-byte aligned.  Everything else is the tangent bundle's contract: origins, origin_per_ray, dirs, s,
 * ns, s_per_ray as in the transmittance bundles; the stream rules (everything enqueued on hip_stream, no host wait, no allocation once
 * a bundle of this size has been seen), the buffers that only grow, the shared queue / counters / scratch slots / bitmap, "counts as a
 * frame in flight"; vrt_hip_get_ray_stats / vrt_hip_get_ray_index_stats report for the same rays every field a radiance bundle
 * reports.  nrays == 0, ns == 0 or a scene of no Gaussians returns VRT_HIP_OK with nothing launched and nothing written; NULL origins,
 * dirs, s or out with work to do, all three inputs NULL, wrt outside the two modes, depth mode with s_per_ray == 0, more than
 * 2^32 - 16 rays, an nrays * ns that does not fit, or an unsupported pair: VRT_HIP_ERR_INVALID with a message, nothing enqueued.  The
 * host form stages s, the three inputs and out in context buffers that only grow and waits once. */
int vrt_hip_transmittance_bundle_tangent_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                                const float *d_s, size_t ns, int s_per_ray, int wrt,
                                                const float *d_tangent      /* N rows of VRT_HIP_GRAD_STRIDE, or NULL */,
                                                const float *d_ray_tangent  /* nrays rows of VRT_HIP_RAY_GRAD_STRIDE, or NULL */,
                                                const float *d_s_tangent    /* nrays * ns, or ns when s_tangent_per_ray == 0, or NULL */,
                                                int s_tangent_per_ray, float *d_out /* nrays * ns, STORED */, void *hip_stream);
int vrt_hip_transmittance_bundle_tangent(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                                         const float *s, size_t ns, int s_per_ray, int wrt, const float *tangent, const float *ray_tangent,
                                         const float *s_tangent, int s_tangent_per_ray, float *out);   /* host pointers, waits */
/* -------- ordered gradient tables: reproducible bits, no float atomics --------------------------------------------------------------
 * Off by default (first value from VRT_HIP_GRAD_ORDERED=0|1 at vrt_hip_create).  With on != 0 all eight gradient entry points above
 * that are given a table (d_grad / grad_out) build it without a single float atomic add, into the table or into any staging memory,
 * and the table is a function of (rays, their order, inputs, scene, options, the table's contents before) alone: bit for bit the same
 * from run to run, with the Morton index on or off, host or device form, with or without ray rows or statistics, on any stream.  No
 * signature changes; ray rows, grad_s and every statistic of vrt_hip_get_ray_stats / vrt_hip_get_ray_index_stats are what the same
 * call gives with the switch off, bit for bit and field for field.  A call without a table (ray rows or grad_s alone) is the call above.
 * What an ordered call enqueues on the caller's stream:
 *   1. count   the cull alone: the length of every ray's kept list;
 *   2. place   every ray gets a range of records -- one per kept Gaussian, two for a ray of the radiance gradient that keeps more than
 *              32 -- by an exclusive scan in ray order.  The total goes to the host: AN ORDERED CALL WAITS ONCE HERE for its stream (the
 *              sort takes its size on the host and the record buffers may have to grow), also in the _device forms, which therefore
 *              cannot be captured into a graph; with the switch off no _device form ever waits.  A total above 2^32 - 1 records is
 *              refused with VRT_HIP_ERR_INVALID, an allocation that fails with VRT_HIP_ERR_HIP: the table is untouched and nothing
 *              further is enqueued.  A total of 0 (no ray keeps anything) runs the kernels of the switch off, which then add nothing;
 *   3. record  the gradient kernels, storing what they add with the switch off as records (Gaussian index, ray id, 9 floats = columns
 *              0..8 of the table, columns nobody computes 0): one per list position of a ray that keeps at most 32; per kept Gaussian
 *              of a longer ray an emitter record and an absorber record (radiance gradient) or one record (transmittance gradient).
 *              A long ray whose second cull does not give the counted length files nothing, and counts as a mismatch (never seen; the
 *              host forms return VRT_HIP_ERR_HIP with a message on one, vrt_hip_get_grad_ordered_stats reports them);
 *   4. sort    a stable radix sort by Gaussian index: the CONSUMED ORDER is (Gaussian, ray id, the record's place in its ray);
 *   5. reduce  NORMATIVE.  For Gaussian j with records rho_0 .. rho_{m-1} in consumed order and each column c: a_l = (((+0.0f +
 *              rho_l[c]) + rho_{l+64}[c]) + rho_{l+128}[c]) + ... for l = 0..63 (+0.0f where there is no record); then six steps s = 1,
 *              2, 4, 8, 16, 32 in this order, each a_l <- a_l + a_{l xor s} from the values before the step; then table[j, c] <-
 *              table[j, c] + a_0.  Plain float32 adds.  Columns 0..8 for a radiance gradient, 4..8 for a transmittance gradient; rows of
 *              Gaussians without records, columns 9..11 and (transmittance gradient) 0..3 are not written at all.
 * The ordered table agrees with the atomic one within the rounding of either.  A segment of m records is summed ceil(m / 64) + 6 adds
 * deep, so its rounding grows like that depth times 2^-24 times the sum of the absolute addends: harmless at thousands of rays per
 * Gaussian, not at millions.  Memory: 56 B per record (key, ray id, 9 floats, and the sort's three words) plus the sort's temporary
 * storage and 20 B per ray, in buffers of the context that only grow.  The call waits for bundles in flight, counts as a state change
 * (vrt_hip_state_generation) and is carried over by vrt_hip_copy_state. */
int vrt_hip_set_grad_ordered(vrt_hip_ctx *ctx, int on);
/* The records of the last ordered call in consumed order, sentinel rows of mismatched rays left out: gauss[i], ray[i] and rows[9 * i ..
 * 9 * i + 8] for i < *count; what the table was reduced from (per-ray gradient rows for Gauss-Newton or per-ray clipping).  Waits for the
 * call.  Before any ordered call, or after one that kept nothing or was refused: *count = 0.  cap (the room in each array, in records)
 * smaller than the count: VRT_HIP_ERR_INVALID with *count set, nothing copied; with cap == 0 the arrays may be NULL. */
int vrt_hip_get_grad_records(vrt_hip_ctx *ctx, uint32_t *gauss, uint32_t *ray, float *rows /* [cap * 9] */, size_t cap, size_t *count);
typedef struct {
    uint64_t records;        /* records reduced into the table (sentinel rows not counted)                          */
    uint64_t gaussians;      /* Gaussians with at least one record: the rows of the table that were written         */
    uint64_t longest;        /* records of the longest segment                                                      */
    uint64_t mismatches;     /* rays whose second cull missed the counted length (0, or the call's table is short)  */
} vrt_hip_grad_ordered_stats;
int vrt_hip_get_grad_ordered_stats(vrt_hip_ctx *ctx, vrt_hip_grad_ordered_stats *out); /* of the last ordered call (waits for it); zeros before any */
typedef struct {
    uint64_t rays;           /* rays of the bundle                                                                  */
    uint64_t short_rays;     /* shaded lane = ray (list of at most 32)                                              */
    uint64_t long_rays;      /* shaded one wave per ray                                                             */
    uint64_t lane_entries;   /* sum over the short rays of the list length                                          */
    uint64_t lane_pairs;     /* sum over the short rays of (list length)^2: their (emitter, absorber) pairs          */
    uint64_t chunks_tested;  /* sum over rays of the chunk spheres (64 Gaussians each) tested                        */
    uint64_t chunks_kept;    /* ... and of those the ray's line reaches                                             */
    uint64_t members_tested; /* sum over rays of the Gaussians tested one by one (members of chunks its WAVE kept)    */
    uint64_t scratch_rays;   /* long rays with more than 1024 kept Gaussians (list continued in device memory)      */
} vrt_hip_ray_stats;
int vrt_hip_get_ray_stats(vrt_hip_ctx *ctx, vrt_hip_ray_stats *out);   /* of the last bundle, when vrt_hip_enable_stats is on (waits for it) */
/* Spatial index of the ray bundles (replaces nothing in the reference, which has no such path; off by default, first value from
 * VRT_HIP_RAY_INDEX=0|1 at vrt_hip_create).  Without it a bundle's only bounding volumes are spheres over runs of 64 CONSECUTIVE
 * Gaussians, which in a scene that is not laid out along a space-filling curve are as large as the scene: nearly every one is kept and
 * every Gaussian is tested against every wave of rays.  With on != 0 the bundles cull through a two-level index instead: the Gaussians
 * in the Morton order of their centres (10 bits per axis over the centres' bounding box, ties by scene index), leaf spheres over 64
 * consecutive positions of that order, group spheres over 64 consecutive leaves, both with the radius that includes the members' cull
 * reach.  Results do not change: the spheres drop only what the per-Gaussian rule above drops, and a ray's list is put back into
 * ascending scene order before it is shaded, so radiance and packed pixels are the same bit for bit, the same rays go to the same
 * kernel, and rays / short_rays / long_rays / lane_entries / lane_pairs / scratch_rays of vrt_hip_ray_stats are the same numbers
 * (its chunk fields are 0 for an indexed bundle: vrt_hip_ray_index_stats below has their counterparts).
 * The index depends on the scene and cull_eps alone: it is made with the scene tables (or by the first bundle after it was switched
 * on), on the host from the centres read back -- for a scene of vrt_hip_set_gaussians_device on the device, the same index -- and never
 * per bundle.  Costs 36 B per Gaussian of device memory plus one bit per
 * Gaussian and workgroup of the one-wave-per-ray kernel.  The call waits for bundles in flight, counts as a state change
 * (vrt_hip_state_generation) and is carried over by vrt_hip_copy_state, whose mirror builds the same index. */
int vrt_hip_set_ray_index(vrt_hip_ctx *ctx, int on);
typedef struct {
    uint64_t indexed;        /* 1: the last bundle culled through the index (all other fields are 0 when it did not)   */
    uint64_t groups;         /* group spheres of the scene: ceil(leaves / 64)                                          */
    uint64_t leaves;         /* leaf spheres of the scene: ceil(N / 64)                                                */
    uint64_t groups_tested;  /* sum over rays of the group spheres tested (all of them)                                */
    uint64_t groups_kept;    /* ... and of those the ray's OWN test keeps                                              */
    uint64_t leaves_tested;  /* sum over rays of the leaf spheres tested (the leaves of groups its WAVE kept)            */
    uint64_t leaves_kept;    /* sum over rays of the leaves its OWN group and leaf tests keep                           */
    uint64_t members_tested; /* sum over rays of the Gaussians tested one by one (members of leaves its WAVE kept)       */
} vrt_hip_ray_index_stats;
int vrt_hip_get_ray_index_stats(vrt_hip_ctx *ctx, vrt_hip_ray_index_stats *out); /* of the last bundle, when vrt_hip_enable_stats is on (waits for it) */
/* Diagnostic: out[Morton position] = scene index, N words (cap = room in out).  Brings the scene tables up to date and waits for work in
 * flight; VRT_HIP_ERR_INVALID when the index is off or not built yet (switched on after the tables: the next bundle builds it). */
int vrt_hip_get_ray_index_perm(vrt_hip_ctx *ctx, uint32_t *out, size_t cap);
/* Sorted bundles (off by default, first value from VRT_HIP_RAY_SORT=0|1 at vrt_hip_create).  A wave of the lane = ray kernels tests the
 * members of every sphere that SOME of its 64 rays keeps, so rays that are neighbours in the bundle but not in space (probes, second
 * bounces, a shuffled batch of pixels) pay for each other's spheres, with or without the index.  With on != 0 every bundle of more than
 * 64 rays -- radiance, transmittance, depth, both gradients, host and device forms, ordered tables included -- is shaded in an order
 * that puts rays which keep the same spheres into the same wave.  Every output word stays at the caller's ray index and every bit stays
 * the same: a ray's bits are a function of (ray, scene, options), whatever its wave-mates are (only a gradient table summed with float
 * atomics differs as it does between any two runs).
 *   Key of ray r, 32 bits: (min(first, 0xFFFF) << 16) | min(last, 0xFFFF), where first and last are the lowest and the highest sphere
 *   that the ray's OWN sphere tests keep -- leaf spheres in Morton position (own group test && own leaf test) with the index on, chunk
 *   spheres with it off; 0xFFFFFFFF for a ray that keeps no sphere.  A function of (ray, scene, options) alone; no member test.
 *   Order: ascending key, equal keys in ascending ray id (a stable sort) -- a function of (rays, scene, options).
 *   Cost: one kernel lane = ray over the bundle's own order (the sphere tests of the cull and nothing below them; with the index its
 *   waves visit the leaf spheres of every group some lane keeps) and one radix sort of nrays (key, id) pairs (over the bits the scene's
 *   sphere count needs: the keys are filed packed, in the same order, and vrt_hip_get_ray_order unpacks them), both on the call's stream
 *   ahead of the bundle's kernels; 16 B per ray of device memory plus the sort's temporary storage, owned by the context, growing only.
 *   A sorted call whose buffers need not grow waits for nothing and allocates nothing.  A bundle that arrives in a coherent order
 *   (a camera's rows) pays the two steps for nothing.
 * A bundle of at most 64 rays is one wave: it is not sorted, and `sorted` says so.  With vrt_hip_enable_stats on, the per-WAVE fields
 * (members_tested and leaves_tested of vrt_hip_ray_stats / vrt_hip_ray_index_stats) count the waves of the sorted order; all per-ray
 * fields (rays, short_rays, long_rays, lane_entries, lane_pairs, scratch_rays, chunks_tested, chunks_kept, groups_tested, groups_kept,
 * leaves_kept) are unchanged.  The call waits for bundles in flight, counts as a state change (vrt_hip_state_generation) and is carried
 * over by vrt_hip_copy_state. */
int vrt_hip_set_ray_sort(vrt_hip_ctx *ctx, int on);
typedef struct {
    uint64_t sorted;              /* 1: the last bundle was shaded in the sorted order (0: switch off, or at most 64 rays)      */
    uint64_t rays;                /* rays of the last bundle                                                                    */
    uint64_t rays_without_sphere; /* of a sorted bundle: rays whose own tests keep no sphere (key 0xFFFFFFFF, sorted last)       */
} vrt_hip_ray_sort_stats;
int vrt_hip_get_ray_sort_stats(vrt_hip_ctx *ctx, vrt_hip_ray_sort_stats *out); /* of the last bundle (waits for a sorted one); needs no vrt_hip_enable_stats */
/* Diagnostic: the last bundle's order[slot] = ray id (lane l of wave w took ray order[64 w + l]) and, where keys != NULL, keys[ray id];
 * *count = its rays, cap = room in each array.  Waits for the bundle.  VRT_HIP_ERR_INVALID when the switch is off or the last bundle
 * was not sorted. */
int vrt_hip_get_ray_order(vrt_hip_ctx *ctx, uint32_t *order, uint32_t *keys, size_t cap, size_t *count);
/* Ray plans: cull a bundle once, reuse its kept lists in every call (replaces nothing in the reference, which has no such path).
 * Every bundle call above -- radiance, transmittance, depth, both gradients and their _rays forms, both tangents, host and device form --
 * begins with the cull of its rays: sphere tests, member tests, the queue of the long rays and their re-cull, with vrt_hip_set_ray_sort
 * the key kernel and the sort, with vrt_hip_set_grad_ordered a count pass that is one more cull.  A loop that sends the same rays
 * through the same scene many times (conjugate gradients on J and J^T, a forward and a backward, a depth bundle and its gradient) pays
 * for the same lists each time.  A plan is that cull run ONCE and kept in device memory; while it is bound, every bundle call takes
 * every ray's list from it and returns the same bits.
 *   Create.  vrt_hip_ray_plan_create_device runs the cull the bundles run (the same text, through the Morton index when
 *   vrt_hip_set_ray_index is on; with vrt_hip_set_ray_sort on and more than 64 rays the key kernel and the sort first, and the plan keeps
 *   the order) on `hip_stream`: a count pass and a scan, ONE wait for the totals, then a fill pair that copies every list out.  It waits
 *   for its stream before it returns, so the plan is complete and may be used on any stream.  Stored per ray: the list length, where the
 *   list begins, the list in ascending scene order (scene indices); the ids of the rays whose list is longer than 32; for a sorted plan
 *   the order and the keys.  4 B per kept entry and per long ray plus 12 B per ray (20 B for a sorted plan); info.bytes has the size.
 *   More than 2^32 - 1 kept entries, more than 2^32 - 16 rays, NULL rays with nrays > 0: VRT_HIP_ERR_INVALID and no plan.  nrays == 0 and
 *   a scene of no Gaussians give legal plans of nothing.  vrt_hip_ray_plan_create is the same from host pointers (on the context's
 *   stream).  The plan belongs to the context: vrt_hip_destroy frees those that are left, vrt_hip_copy_state carries neither plans nor
 *   the binding, and every call below refuses (VRT_HIP_ERR_INVALID) a plan of another context.
 *   Bind.  vrt_hip_set_ray_plan(ctx, plan, flags) binds a plan (NULL: none); it and vrt_hip_ray_plan_destroy wait for bundles in flight,
 *   as the other switches do, and destroying the bound plan unbinds it.  While a plan is bound a bundle call runs no sphere test, no
 *   member test, no filing into the queue, no key kernel, no sort, and uses no scratch slot and no bitmap: a ray with more than 32
 *   entries goes to the one-wave-per-ray kernel as it would have, which takes the plan's queue, copies the first 1024 entries to LDS and
 *   reads the rest where they stand.  The lane = ray kernels take the plan's order; the context's index and sort switches are ignored
 *   (flipping them changes no bit and does not make a plan stale).  With vrt_hip_set_grad_ordered on, the count pass is the plan's
 *   lengths and `mismatches` is 0 by construction.  The stream rules are unchanged -- the long kernel's work counter is still the
 *   context's, so two bundles of one context are ordered by the stream they share -- and a planned call whose buffers need not grow
 *   waits for nothing and allocates nothing, but for the ordered call's own wait.
 *   Contract of a planned call.  nrays must be the plan's: otherwise VRT_HIP_ERR_INVALID with both numbers, nothing enqueued.  The
 *   caller still passes the rays -- the plan does not own them -- and which rays those are is the caller's business: other rays than
 *   the plan's give the sum over the plan's lists, which is defined and no error.  With flags == 0 the plan is STRICT: a call made after
 *   the Gaussians were set again (vrt_hip_set_gaussians*, vrt_hip_set_gaussians_device, vrt_hip_copy_state into the context), or after
 *   cull_eps or the Exp / Erf pair changed (vrt_hip_set_options), returns VRT_HIP_ERR_INVALID with a message that says which, nothing
 *   enqueued.  With VRT_HIP_PLAN_KEEP_LISTS the lists stay in force across such updates while the scene keeps its size N (another N:
 *   VRT_HIP_ERR_INVALID -- the entries are scene indices): the call computes the sum over the plan's lists for the CURRENT scene and the
 *   rays given.  Nothing is dropped and nothing new is picked up: that is the function whose derivative the gradient and tangent
 *   bundles return ("each ray's kept list is held fixed"), so a line search, a finite difference or a trial step along a tangent
 *   evaluates the function whose J was used.
 *   Statistics of a planned call.  rays, short_rays, long_rays, lane_entries, lane_pairs and scratch_rays of vrt_hip_ray_stats are the
 *   unplanned call's; chunks_tested, chunks_kept and members_tested are 0; vrt_hip_get_ray_index_stats reads indexed = 0 and zeros;
 *   vrt_hip_get_ray_sort_stats.sorted is the plan's flag (rays_without_sphere: 0, a plan does not keep it) and vrt_hip_get_ray_order
 *   gives the plan's order and keys, whatever the sort switch says.
 * Out of scope: the camera / frame path, the multi-GPU group, plans that follow a changing N, noticing that the rays differ from the
 * plan's, graph capture. */
typedef struct vrt_hip_ray_plan vrt_hip_ray_plan;
#define VRT_HIP_PLAN_KEEP_LISTS 1
typedef struct {
    uint64_t rays;           /* rays of the plan                                                                     */
    uint64_t entries;        /* kept (ray, Gaussian) pairs: the sum of the list lengths                              */
    uint64_t short_rays;     /* rays with a list of at most 32: shaded lane = ray                                    */
    uint64_t long_rays;      /* rays with a longer list: shaded one wave per ray                                     */
    uint64_t longest;        /* the longest list                                                                     */
    uint64_t scratch_rays;   /* rays with more than 1024 kept Gaussians (the list continues in the plan's memory)    */
    uint64_t bytes;          /* device memory of the plan                                                            */
    uint64_t sorted;         /* 1: made with vrt_hip_set_ray_sort on and more than 64 rays; the plan keeps the order  */
    uint64_t indexed;        /* 1: made through the Morton index (the same lists either way)                         */
    uint64_t scene_n;        /* Gaussians of the scene it was made for                                               */
    uint64_t cull_generation; /* the context's count of scene and cull-option changes at creation                    */
} vrt_hip_ray_plan_info;
int vrt_hip_ray_plan_create_device(vrt_hip_ctx *ctx, size_t nrays, const float *d_origins, int origin_per_ray, const float *d_dirs,
                                   void *hip_stream, vrt_hip_ray_plan **out);
int vrt_hip_ray_plan_create(vrt_hip_ctx *ctx, size_t nrays, const float *origins, int origin_per_ray, const float *dirs,
                            vrt_hip_ray_plan **out);
int vrt_hip_ray_plan_destroy(vrt_hip_ctx *ctx, vrt_hip_ray_plan *plan);
int vrt_hip_set_ray_plan(vrt_hip_ctx *ctx, vrt_hip_ray_plan *plan, int flags);
int vrt_hip_get_ray_plan_info(vrt_hip_ctx *ctx, vrt_hip_ray_plan *plan, vrt_hip_ray_plan_info *out);
/* Read-out: offsets[nrays + 1] and, where entries != NULL, the info.entries kept scene indices: ray r (the caller's index) keeps
 * entries[offsets[r] .. offsets[r + 1]), ascending. */
int vrt_hip_get_ray_plan_lists(vrt_hip_ctx *ctx, vrt_hip_ray_plan *plan, uint64_t *offsets, uint32_t *entries);

/* Numeric cross-checks of rt.cpp:8-27 (transmittance_step uses fast_exp like the reference).
 * vrt_hip_transmittance_step runs the reference's float32 loop `for (t = 0; t <= s; t += delta)` per sample point, and refuses with
 * VRT_HIP_ERR_INVALID (and a reason in vrt_hip_last_error), before anything is uploaded or launched, the arguments with which that loop
 * does not end or holds the GPU for long:
 *   - delta that is not a normal positive float (0, negative, NaN, below FLT_MIN);
 *   - any s[k] = +inf;
 *   - max finite s[k] >= delta * 2^23: from there on t + delta rounds back to t (delta = 0.01: s >= 83,886.08);
 *   - ceil(max s[k] / delta) * max(n, 1) > 2^23 density evaluations in one lane, n the number of Gaussians (about a second).
 * Negative and NaN sample points are accepted and behave as in the reference: zero steps, T = fast_exp(-0).
 * csrc/vrt_step_guard.hpp has the predicate and the proof that an accepted call ends. */
int vrt_hip_transmittance_step(vrt_hip_ctx *ctx, const float o[3], const float n[3], const float *s, size_t ns,
                               float delta, float *T_out);
int vrt_hip_density(vrt_hip_ctx *ctx, size_t npts, const float *pts, float *D_out);

/* -------- elementwise approximations (approx.cpp) on device; for the accuracy study ------ */
int vrt_hip_eval_erf(vrt_hip_ctx *ctx, int erf_kind, const float *x, size_t n, float *y);
int vrt_hip_eval_exp(vrt_hip_ctx *ctx, int exp_kind, const float *x, size_t n, float *y);

/* Table mode for dense scenes (ON by default; NOT the reference's summation order, but inside its tolerance by a bound the
 * kernel checks per ray): blocks with many overlapping Gaussians evaluate the transmittance exponent of a ray at up to 384
 * equidistant nodes along it and interpolate the 5 n sample points (n * G erf terms per ray instead of 5 n^2).
 * `step` = requested node spacing in units of sqrt2 * sigma of the narrowest Gaussian of the block (default 0.05; 0 = off:
 * the exact kernels only, which reproduce the reference's per-term sums).  Every ray's worst-case radiance change --
 * sum over its samples of |term| * (0.0212 u^2 * K + 0.36 u^4 * S_all), see render_table_body in csrc/vrt_table_kernel.hip --
 * must stay below the budget (default 2.5e-5), or the block is redone at 0.6 of the spacing and then shaded exactly; so
 * are blocks with more than 2048 survivors.
 * Applies to the Exp / Erf pairs {vcl_exp, expf} x {A&S erf, erff}; other pairs are always exact. */
int vrt_hip_set_table_step(vrt_hip_ctx *ctx, float step);
int vrt_hip_set_table_budget(vrt_hip_ctx *ctx, float budget);

/* Budgeted ray-level cull of the one-wave ("block") kernel.  `cull_eps` (vrt_hip_set_options; replaces nothing in the reference,
 * which sums every Gaussian of a tile: rt.h:205-223) bounds what dropped Gaussians can change by worst-case counting; a ray's own
 * list is additionally cut by the SUM of what it drops: the smallest entries go while sum sigma*mag*exp(-x) <= kappa * 1365 * cull_eps
 * (default kappa 6: the ray's radiance changes by at most 3 * that = 2.46e-5 for albedos <= 1 -- the budget is divided by the scene's
 * largest albedo beyond that; 0 = off; cull_eps = 0 switches every cull off). */
int vrt_hip_set_cull_prune(vrt_hip_ctx *ctx, float kappa);

/* -------- statistics of the last render ----------------------------------------------------- */
typedef struct {
    double kernel_ms;        /* render kernel time of the last vrt_hip_render() (HIP events)       */
    double tiling_ms;        /* last vrt_hip_tile_gaussians() device time                           */
    uint64_t rays;           /* rays shaded                                                         */
    uint64_t blocks;         /* 8x8 pixel blocks (one wavefront each)                                */
    uint64_t list_entries;   /* sum over blocks of candidates kept by the block cull                 */
    uint64_t tile_entries;   /* sum over blocks of the (tile-culled) tile list length they scanned    */
    uint64_t overflow_blocks;/* dense-kernel blocks with more than 1024 survivors (streamed from scratch)      */
    uint64_t lane_entries;   /* sum over rays of the per-ray list length (fast path)                  */
    uint64_t lane_max_entries;/* sum over blocks of the longest per-ray list (the loop trip count)    */
    uint64_t shaded_blocks;  /* blocks that reached the shading loops (the rest were only cleared)    */
    uint64_t dense_blocks;   /* of those, blocks shaded by the 16-waves-per-block kernel              */
    double dense_busy_frac;  /* mean share of that kernel's duration its workgroups had blocks to work on */
    uint64_t table_blocks;   /* of the dense blocks, those shaded through the interpolation table (vrt_hip_set_table_step) */
    uint64_t lane_pairs;     /* sum over rays of (per-ray list length)^2: the (emitter, absorber) pairs the one-wave
                                kernel has to evaluate, 5 erf terms each -- the ALGORITHMIC work of its pair loops    */
    /* dense kernel: visits of an absorber by a chunk of 6 emitters (30 erf terms on every ray of the block when
     * evaluated), split by what the exact saturation tests decided */
    uint64_t dense_visits_full;   /* evaluated term by term                                              */
    uint64_t dense_visits_zero;   /* every term exactly 0 (absorber behind all samples): skipped         */
    uint64_t dense_visits_common; /* every term exactly -2 A_j (absorber in front of all samples): one fma */
    /* table kernel */
    uint64_t table_nodes;     /* sum over its blocks of the node count G                                     */
    uint64_t table_retries;   /* blocks that met the error budget only at the reduced spacing                */
    uint64_t table_skips;     /* (absorber, wave) visits settled by saturation (one add instead of NT terms) */
    uint64_t table_declined;  /* blocks handed to the exact kernel                                           */
    uint64_t table_coarser;   /* blocks done at a coarser spacing than requested (the bound left room)       */
    uint64_t table_empty;     /* of table_blocks, blocks no Gaussian reaches (the rim of a dense cell)       */
    uint64_t table_phase_ticks[8]; /* 10-ns ticks its workgroups spent, summed over blocks: set-up, cull, range, spacing
                                      estimate, kink weights, table, emission, reduction                      */
    uint64_t dense_launch_skips; /* frames of this context whose dense launch was left out (a frame of exactly the same state had
                                    reported that there is nothing for it); counted since the context was created */
} vrt_hip_stats;
int vrt_hip_get_stats(vrt_hip_ctx *ctx, vrt_hip_stats *out);
/* Enables per-block statistics collection (small atomics; off by default). */
int vrt_hip_enable_stats(vrt_hip_ctx *ctx, int on);
/* Kernel timing for roofline reports: while enabled, every render launch is bracketed with HIP events ON THE
 * STREAM IT RUNS ON (ring of the last 512 launches).  get() waits for them and returns the mean duration of
 * the one-wave-per-block render kernel, of the 16-waves-per-block (dense) kernel and of the list kernels.
 * on = 1: four events per frame (all three durations); on = 2: two events, around the one-wave render kernel only
 * (the other two durations read 0) -- an event costs the stream 2-3 us, which matters for 0.06 ms frames;
 * on = 3: like 2, on every 8th frame only. */
int vrt_hip_enable_kernel_timing(vrt_hip_ctx *ctx, int on);
int vrt_hip_get_kernel_timing(vrt_hip_ctx *ctx, double *render_ms, double *dense_ms, double *lists_ms, uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
