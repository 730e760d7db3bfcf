// vrt.hpp -- C++ host-side mirror of the reference's vrt:: interface for the hot path, implemented
// on the C ABI of libvrt_hip.so (include/vrt_hip.h).  Same names, argument meaning and return values as
//   src/vrt/types.h   vec4f_t, simd_vec4f_t, gaussian_t, simd_gaussian_t, gaussian_vec_t, gaussians_t, tiles_t
//   src/vrt/camera.h  camera_t, camera_create_info_t
//   src/vrt/rt.h      transmittance, simd_transmittance, broadcast_transmittance, radiance, simd_radiance,
//                     broadcast_radiance, render_image (2 overloads), simd_render_image (2 overloads),
//                     tile_gaussians, transmittance_step, density
//   src/vrt/gaussians-from-file.h  read_from_obj
// so that the reference's callers (volumetric-ray-tracer/main.cpp:257-296, tests/transmittance.cpp,
// tests/img-error.cpp) compile against it with two mechanical changes:
//   * the Exp/Erf template arguments are tags (vrt::exp_kind / vrt::erf_kind) instead of function
//     pointers -- device code cannot take a host function pointer;
//   * glm::mat4 is replaced by the 16-float column-major array camera_t::view_matrix holds.
// There is no CPU path here: every function forwards to the GPU and throws vrt::hip_error when the
// library reports a failure (the reference _exit(1)s on its assertion failures, definitions.h:23-30).
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../vrt_hip.h"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int8_t i8;
typedef int32_t i32;
typedef float f32;

namespace vrt {

struct hip_error : std::runtime_error { using std::runtime_error::runtime_error; };

// ---- template tags for the reference's Exp / Erf arguments (rt.h:32,61,102; approx.h) ------------
enum class exp_kind : int { libm = VRT_EXP_LIBM, vcl = VRT_EXP_VCL, fast = VRT_EXP_FAST, spline = VRT_EXP_SPLINE };
enum class erf_kind : int { libm = VRT_ERF_LIBM, abramowitz_stegun = VRT_ERF_AS, spline = VRT_ERF_SPLINE,
                            spline_mirror = VRT_ERF_SPLINE_MIRROR, taylor = VRT_ERF_TAYLOR };

// ---- types.h:19-113 ---------------------------------------------------------------------------------
struct vec4f_t {
    f32 x, y, z, w = 0.f;
    vec4f_t operator+(const vec4f_t &o) const { return { x + o.x, y + o.y, z + o.z, w + o.w }; }
    vec4f_t operator-(const vec4f_t &o) const { return { x - o.x, y - o.y, z - o.z, w - o.w }; }
    vec4f_t operator*(const f32 &l) const { return { x * l, y * l, z * l, w * l }; }
    vec4f_t operator/(const vec4f_t &o) const { return { x / o.x, y / o.y, z / o.z, w / o.w }; }
    f32 dot(const vec4f_t &o) const { return x * o.x + y * o.y + z * o.z + w * o.w; }
    f32 sqnorm() const { return dot(*this); }
    void normalize() { const f32 n = std::sqrt(dot(*this)); x /= n; y /= n; z /= n; w /= n; }
};

// ---- types.h:195-229 (40 bytes, the layout vrt_hip_set_gaussians_aos takes) -------------------------
struct gaussian_t {
    vec4f_t albedo;
    vec4f_t mu;
    f32 sigma;
    f32 magnitude;
};
static_assert(sizeof(gaussian_t) == 40, "gaussian_t must match the reference's AoS layout");

// ---- types.h:115-193, 289-306: the W-wide twins.  The reference's W is the host's SIMD width (16 on AVX-512, 8 on
//      AVX2); here a lane is a ray of a wave64, so W = 64 and simd::Vec<simd::Float> is a plain array of 64 floats.
//      They exist so that callers of broadcast_transmittance / broadcast_radiance (rt.h:102-103, 205-206) compile:
//      the arithmetic on them happens on the GPU, one lane per ray.  (simd_gaussian_t::pdf has no host evaluator: the
//      density is evaluated inside the kernels, types.h:299-302 <-> emission_term in csrc/vrt_kernels_common.hpp.) ---------
constexpr u64 SIMD_FLOATS = 64;
namespace simd {
struct Float {};
template <typename T> struct Vec;
template <> struct Vec<Float> {
    std::array<f32, SIMD_FLOATS> v;
    f32 &operator[](size_t i) { return v[i]; }
    const f32 &operator[](size_t i) const { return v[i]; }
};
template <typename T> inline Vec<T> set1(f32 x) { Vec<T> r; r.v.fill(x); return r; }
inline void store(f32 *p, const Vec<Float> &a) { std::memcpy(p, a.v.data(), sizeof a.v); }
inline Vec<Float> load(const f32 *p) { Vec<Float> r; std::memcpy(r.v.data(), p, sizeof r.v); return r; }
} // namespace simd

struct simd_vec4f_t {
    simd::Vec<simd::Float> x, y, z, w = simd::set1<simd::Float>(0.f);
    static simd_vec4f_t from_vec4f_t(const vec4f_t &o) // types.h:183-192
    {
        return { simd::set1<simd::Float>(o.x), simd::set1<simd::Float>(o.y), simd::set1<simd::Float>(o.z), simd::set1<simd::Float>(o.w) };
    }
    vec4f_t lane(size_t i) const { return { x[i], y[i], z[i], w[i] }; }
    void set_lane(size_t i, const vec4f_t &o) { x[i] = o.x; y[i] = o.y; z[i] = o.z; w[i] = o.w; }
};

struct simd_gaussian_t {
    simd_vec4f_t albedo, mu;
    simd::Vec<simd::Float> sigma, magnitude;
    static simd_gaussian_t from_gaussian_t(const gaussian_t &g) // types.cpp:113-121
    {
        return { simd_vec4f_t::from_vec4f_t(g.albedo), simd_vec4f_t::from_vec4f_t(g.mu), simd::set1<simd::Float>(g.sigma),
                 simd::set1<simd::Float>(g.magnitude) };
    }
};

// ---- types.h:232-264: SoA mirror (padded to (n/W+1)*W with sigma 1, magnitude 0; W = 16) --------------
struct gaussian_vec_t {
    struct { std::vector<f32> r, g, b; } albedo;
    struct { std::vector<f32> x, y, z; } mu;
    std::vector<f32> sigma, magnitude;
    u64 size = 0;
    void load_gaussians(const std::vector<gaussian_t> &g)
    {
        for (u64 i = 0; i < size; ++i) {
            const bool pad = i >= g.size();
            mu.x[i] = pad ? 0.f : g[i].mu.x; mu.y[i] = pad ? 0.f : g[i].mu.y; mu.z[i] = pad ? 0.f : g[i].mu.z;
            albedo.r[i] = pad ? 0.f : g[i].albedo.x; albedo.g[i] = pad ? 0.f : g[i].albedo.y; albedo.b[i] = pad ? 0.f : g[i].albedo.z;
            sigma[i] = pad ? 1.f : g[i].sigma; magnitude[i] = pad ? 0.f : g[i].magnitude;
        }
    }
    static gaussian_vec_t *from_gaussians(const std::vector<gaussian_t> &g)
    {
        gaussian_vec_t *v = new gaussian_vec_t();
        v->size = (g.size() / 16 + 1) * 16;
        for (auto *a : { &v->albedo.r, &v->albedo.g, &v->albedo.b, &v->mu.x, &v->mu.y, &v->mu.z, &v->sigma, &v->magnitude }) a->resize(v->size);
        v->load_gaussians(g);
        return v;
    }
};

// ---- types.h:266-270 ------------------------------------------------------------------------------------
struct gaussians_t {
    std::vector<gaussian_t> gaussians;
    gaussian_vec_t *soa_gaussians = nullptr;
};

// ---- types.h:272-287.  The reference's tiles_t OWNS a copy of every tile's Gaussians; here the per-tile sets live on
//      the device as index lists, and the object keeps what is needed to rebuild them (the scene it was made from, the
//      tile size and the view matrix): a tiles_t stays valid whatever the process renders in between -- an untiled
//      render, another scene, another tiling -- the tiled overloads re-bin when the device no longer holds THIS set. ---
struct tiles_t {
    f32 tw, th;
    u64 w, h;
    std::vector<u32> counts; // per tile, row-major: gaussians[t].gaussians.size() of the reference
    std::shared_ptr<const std::vector<gaussian_t>> scene;
    std::array<f32, 16> view;
    mutable u64 generation;  // device state (detail::device_t::generation) that holds this tile set
};

// ---- camera.h:7-44, camera.cpp:7-79 (own 3-vector maths; view_matrix is column-major like glm::mat4) ------
struct camera_create_info_t {
    std::array<f32, 3> position{ 0.f, 0.f, 0.f }, up{ 0.f, 1.f, 0.f }, front{ 0.f, 0.f, 1.f };
    f32 yaw = -90.f, pitch = 0.f;
    u64 width = 256, height = 256;
    f32 focal_length = 1.f;
};

struct camera_t {
    std::array<f32, 3> position, front, up, world_up, right;
    std::array<f32, 16> view_matrix;
    f32 focal_length;
    u64 w, h;
    struct { std::vector<f32> xs, ys, zs; } projection_plane;

    camera_t(std::array<f32, 3> position_, std::array<f32, 3> up_ = { 0.f, 1.f, 0.f }, std::array<f32, 3> front_ = { 0.f, 0.f, 1.f },
             f32 yaw = -90.f, f32 pitch = 0.f, u64 width = 256, u64 height = 256, f32 focal = 1.f)
        : position(position_), front(front_), up(up_), world_up(up_), focal_length(focal), w(width), h(height)
    {
        turn(yaw, pitch);
    }
    explicit camera_t(const camera_create_info_t &ci)
        : camera_t(ci.position, ci.up, ci.front, ci.yaw, ci.pitch, ci.width, ci.height, ci.focal_length) {}

    // camera.cpp:7-23.  The arithmetic is the library's (vrt_hip_camera_*, csrc/vrt_host_camera.cpp): glm's lookAt ->
    // translate -> inverse -> mat4*vec4 in glm's order of operations, compiled once without contraction or fast-math,
    // so the view matrix and the plane points do not depend on the flags THIS header is compiled with -- a last-bit
    // difference in a ray shows up as up to 5e-4 of radiance for small sigma.
    void turn(const f32 yaw, const f32 pitch, const bool constrain = true)
    {
        vrt_hip_camera c = to_c();
        vrt_hip_camera_turn(&c, yaw, pitch, constrain ? 1 : 0);
        from_c(c);
        planes(c);
    }
    // camera.cpp:50-71: view = translate(lookAt(pos, pos + front, up), focal * front); plane = inverse(view) * (x, y, 0, 1)
    void update()
    {
        vrt_hip_camera c = to_c();
        vrt_hip_camera_refresh(&c); // front / right / up as they are (camera_t::update does not re-derive them)
        from_c(c);
        planes(c);
    }
    // main.cpp:252, 330: position = rotate(I, radians(deg), +Y) * position (follow with turn(angle - deg, 0))
    void orbit(const f32 deg)
    {
        vrt_hip_camera c = to_c();
        vrt_hip_camera_orbit(&c, deg);
        for (int i = 0; i < 3; ++i) position[i] = c.position[i];
    }

private:
    vrt_hip_camera to_c() const
    {
        vrt_hip_camera c;
        std::memset(&c, 0, sizeof c);
        for (int i = 0; i < 3; ++i) {
            c.position[i] = position[i]; c.front[i] = front[i]; c.up[i] = up[i]; c.world_up[i] = world_up[i]; c.right[i] = right[i];
        }
        for (int i = 0; i < 16; ++i) c.view[i] = view_matrix[i];
        c.focal_length = focal_length; c.w = w; c.h = h;
        return c;
    }
    void from_c(const vrt_hip_camera &c)
    {
        for (int i = 0; i < 3; ++i) { front[i] = c.front[i]; up[i] = c.up[i]; right[i] = c.right[i]; }
        for (int i = 0; i < 16; ++i) view_matrix[i] = c.view[i];
    }
    void planes(const vrt_hip_camera &c)
    {
        projection_plane.xs.resize(w * h); projection_plane.ys.resize(w * h); projection_plane.zs.resize(w * h);
        vrt_hip_camera_plane(&c, projection_plane.xs.data(), projection_plane.ys.data(), projection_plane.zs.data());
    }
};

// ---- the process-wide device context behind the free functions -------------------------------------------------
namespace detail {
struct device_t {
    vrt_hip_ctx *ctx = nullptr;
    const void *scene_key = nullptr; // identity of the last uploaded Gaussian vector
    size_t scene_n = 0;
    u64 scene_hash = 0;
    u64 generation = 0;   // bumped whenever the device's scene or tile sets change: names what the device holds
    const f32 *plane_key = nullptr;
    u64 plane_w = 0, plane_h = 0;
    f32 cull_eps = 1e-9f;

    static device_t &get()
    {
        static device_t d;
        if (!d.ctx) {
            const char *dev = std::getenv("VRT_HIP_DEVICE");
            if (vrt_hip_create(dev ? std::atoi(dev) : 0, &d.ctx) != VRT_HIP_OK)
                throw hip_error(std::string("vrt_hip_create: ") + vrt_hip_last_error(nullptr));
            if (const char *e = std::getenv("VRT_HIP_CULL_EPS")) d.cull_eps = (f32)std::atof(e);
        }
        return d;
    }
    void check(int rc, const char *what) const
    {
        if (rc != VRT_HIP_OK) throw hip_error(std::string(what) + ": " + vrt_hip_last_error(ctx));
    }
    static u64 hash(const std::vector<gaussian_t> &g)
    {
        u64 h = 1469598103934665603ull;
        const unsigned char *p = reinterpret_cast<const unsigned char *>(g.data());
        for (size_t i = 0; i < g.size() * sizeof(gaussian_t); ++i) { h ^= p[i]; h *= 1099511628211ull; }
        return h;
    }
    bool device_scene = false; // the scene came from device memory (vrt::set_gaussians_device): an EMPTY vector stands for it
    void upload_scene(const std::vector<gaussian_t> &g)
    {
        if (device_scene && g.empty()) return;
        device_scene = false;
        const u64 h = hash(g);
        if (scene_n == g.size() && scene_hash == h && scene_key) return;
        check(vrt_hip_set_gaussians_aos(ctx, g.size(), g.data()), "vrt_hip_set_gaussians_aos");
        scene_key = g.data(); scene_n = g.size(); scene_hash = h;
        ++generation; // tile sets of the old scene are gone
    }
    void upload_plane(const camera_t &cam)
    {
        check(vrt_hip_set_plane(ctx, (u32)cam.w, (u32)cam.h, cam.projection_plane.xs.data(), cam.projection_plane.ys.data(),
                                cam.projection_plane.zs.data()), "vrt_hip_set_plane");
    }
    void untiled()
    {
        check(vrt_hip_clear_tiles(ctx), "vrt_hip_clear_tiles");
        ++generation;
    }
    void options(exp_kind e, erf_kind r) { check(vrt_hip_set_options(ctx, (int)e, (int)r, cull_eps), "vrt_hip_set_options"); }
};
} // namespace detail

// ---- rt.h:140 / rt.cpp:29-69.  The reference passes glm::mat4; here the camera's 16 floats.  The tile sets stay
//      on the device (index lists); the returned object carries their sizes and names the device-side set. -----
inline tiles_t tile_gaussians(const f32 tw, const f32 th, const std::vector<gaussian_t> &gaussians, const std::array<f32, 16> &view)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians);
    d.check(vrt_hip_tile_gaussians(d.ctx, tw, th, view.data()), "vrt_hip_tile_gaussians");
    tiles_t t{ tw, th, 0, 0, {}, std::make_shared<const std::vector<gaussian_t>>(gaussians), view, ++d.generation };
    d.check(vrt_hip_get_tile_counts(d.ctx, nullptr, 0, &t.w, &t.h), "vrt_hip_get_tile_counts");
    t.counts.resize(t.w * t.h);
    d.check(vrt_hip_get_tile_counts(d.ctx, t.counts.data(), t.counts.size(), nullptr, nullptr), "vrt_hip_get_tile_counts");
    return t;
}

namespace detail {
inline bool render(u32 width, u32 height, u32 *image, const camera_t &cam, const vec4f_t &origin, int pack, exp_kind e, erf_kind r,
                   const bool &running)
{
    if (!running) return true;
    auto &d = device_t::get();
    if (cam.w != width || cam.h != height) throw hip_error("render: camera size differs from image size");
    d.upload_plane(cam);
    d.options(e, r);
    const f32 o[3] = { origin.x, origin.y, origin.z };
    d.check(vrt_hip_render(d.ctx, o, pack, image, nullptr), "vrt_hip_render");
    return !running; // the reference returns true when the viewer asked to stop (rt.h:244, 308, 334, 402)
}
// make the device hold `tiles` (its scene and its tile sets) before a tiled render
inline void bind_tiles(const tiles_t &tiles)
{
    auto &d = device_t::get();
    if (tiles.generation == d.generation) return;
    if (!tiles.scene) throw hip_error("tiles_t was not made by vrt::tile_gaussians");
    d.upload_scene(*tiles.scene);
    d.check(vrt_hip_tile_gaussians_device(d.ctx, tiles.tw, tiles.th, tiles.view.data(), nullptr), "vrt_hip_tile_gaussians");
    tiles.generation = ++d.generation;
}
} // namespace detail

// ---- rt.h:227-247: scalar render, untiled: truncating pack, opaque alpha ------------------------------------------
template <exp_kind Exp = exp_kind::libm, erf_kind Erf = erf_kind::libm>
bool render_image(const u32 width, const u32 height, u32 *image, const camera_t &cam, const vec4f_t &origin,
                  const gaussians_t &gaussians, const bool &running = true)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.untiled();
    return detail::render(width, height, image, cam, origin, VRT_PACK_TRUNC | VRT_ALPHA_OPAQUE, Exp, Erf, running);
}
// ---- rt.h:251-310: scalar render, tiled (tc = thread count: the GPU grid replaces the pool) -----------------------
template <exp_kind Exp = exp_kind::libm, erf_kind Erf = erf_kind::libm>
bool render_image(const u32 width, const u32 height, u32 *image, const camera_t &cam, const vec4f_t &origin,
                  const tiles_t &tiles, const bool &running, const u64 /*tc*/)
{
    detail::bind_tiles(tiles);
    return detail::render(width, height, image, cam, origin, VRT_PACK_TRUNC | VRT_ALPHA_OPAQUE, Exp, Erf, running);
}
// ---- rt.h:315-337: SIMD-over-pixels render, untiled: rounding pack, opaque alpha ----------------------------------
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
bool simd_render_image(const u32 width, const u32 height, u32 *image, const camera_t &cam, const vec4f_t &origin,
                       const gaussians_t &gaussians, const bool &running = true)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.untiled();
    return detail::render(width, height, image, cam, origin, VRT_PACK_ROUND | VRT_ALPHA_OPAQUE, Exp, Erf, running);
}
// ---- rt.h:344-404: SIMD-over-pixels render, tiled (the CLI default, mode 8): rounding pack, computed alpha --------
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
bool simd_render_image(const u32 width, const u32 height, u32 *image, const camera_t &cam, const vec4f_t origin,
                       const tiles_t &tiles, const bool &running, const u64 /*tc*/)
{
    detail::bind_tiles(tiles);
    return detail::render(width, height, image, cam, origin, VRT_PACK_ROUND | VRT_ALPHA_COMPUTED, Exp, Erf, running);
}

// ---- rt.h:32-54 (and its SIMD twins rt.h:61-127, which compute the same function) -----------------------------------
template <exp_kind Exp = exp_kind::libm, erf_kind Erf = erf_kind::libm>
f32 transmittance(const vec4f_t o, const vec4f_t n, const f32 s, const gaussians_t &gaussians)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    const f32 oo[3] = { o.x, o.y, o.z }, nn[3] = { n.x, n.y, n.z };
    f32 T = 0.f;
    d.check(vrt_hip_transmittance(d.ctx, oo, nn, &s, 1, &T), "vrt_hip_transmittance");
    return T;
}
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
f32 simd_transmittance(const vec4f_t o, const vec4f_t n, const f32 s, const gaussians_t &g) { return transmittance<Exp, Erf>(o, n, s, g); }
// ---- rt.h:102-127: SIMD_FLOATS rays at once, each with its own origin, direction and sample point -------------------
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
simd::Vec<simd::Float> broadcast_transmittance(const simd_vec4f_t &o, const simd_vec4f_t &n, const simd::Vec<simd::Float> &s,
                                               const gaussians_t &gaussians)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    f32 oo[3 * SIMD_FLOATS], nn[3 * SIMD_FLOATS];
    for (u64 l = 0; l < SIMD_FLOATS; ++l) {
        oo[3 * l] = o.x[l]; oo[3 * l + 1] = o.y[l]; oo[3 * l + 2] = o.z[l];
        nn[3 * l] = n.x[l]; nn[3 * l + 1] = n.y[l]; nn[3 * l + 2] = n.z[l];
    }
    simd::Vec<simd::Float> T;
    d.check(vrt_hip_transmittance_rays(d.ctx, SIMD_FLOATS, oo, nn, s.v.data(), T.v.data()), "vrt_hip_transmittance_rays");
    return T;
}

// ---- rt.h:146-164 / 166-199 / 205-223: L_hat incl. w = sum albedo.w * inner ------------------------------------------
template <exp_kind Exp = exp_kind::libm, erf_kind Erf = erf_kind::libm>
vec4f_t radiance(const vec4f_t o, const vec4f_t n, const gaussians_t &gaussians)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    const f32 oo[3] = { o.x, o.y, o.z }, nn[3] = { n.x, n.y, n.z };
    f32 out[4];
    d.check(vrt_hip_radiance(d.ctx, 1, oo, nn, out), "vrt_hip_radiance");
    return { out[0], out[1], out[2], out[3] };
}
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
vec4f_t simd_radiance(const vec4f_t o, const vec4f_t n, const gaussians_t &g) { return radiance<Exp, Erf>(o, n, g); }
// ---- rt.h:205-223: SIMD_FLOATS rays at once (lane = ray); the kernel the tiled renderer runs per pixel vector --------
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
simd_vec4f_t broadcast_radiance(const simd_vec4f_t o, const simd_vec4f_t n, const gaussians_t &gaussians)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    f32 oo[3 * SIMD_FLOATS], nn[3 * SIMD_FLOATS], out[4 * SIMD_FLOATS];
    for (u64 l = 0; l < SIMD_FLOATS; ++l) {
        oo[3 * l] = o.x[l]; oo[3 * l + 1] = o.y[l]; oo[3 * l + 2] = o.z[l];
        nn[3 * l] = n.x[l]; nn[3 * l + 1] = n.y[l]; nn[3 * l + 2] = n.z[l];
    }
    d.check(vrt_hip_radiance(d.ctx, SIMD_FLOATS, oo, nn, out), "vrt_hip_radiance");
    simd_vec4f_t L;
    for (u64 l = 0; l < SIMD_FLOATS; ++l) L.set_lane(l, { out[4 * l], out[4 * l + 1], out[4 * l + 2], out[4 * l + 3] });
    return L;
}

// ======== EXTENSION -- not in the reference ===========================================================================
// Ray bundles: broadcast_radiance for ANY number of rays in ONE call, culled per ray (vrt_hip_radiance_rays in
// include/vrt_hip.h: a ray loses less than 3 * cull_eps * min(N, 4096) = 1.23e-5 of radiance at the defaults).  Ray r has
// origin o[r] and unit direction n[r] (normalised by the caller); out[r] = its radiance (x, y, z = rgb, w = sum albedo.w *
// inner); image (nullable): one packed pixel per ray.  A stereo pair, a fisheye, light probes or a second bounce are one
// call each.  vrt::radiance / broadcast_radiance above stay the reference's full sum.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays(const vec4f_t *o, const vec4f_t *n, size_t nrays, const gaussians_t &gaussians, vec4f_t *out, u32 *image = nullptr,
                   int pack_flags = VRT_PACK_ROUND | VRT_ALPHA_COMPUTED)
{
    static_assert(sizeof(vec4f_t) == 4 * sizeof(f32), "out is handed to the library as 4 floats per ray");
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    std::vector<f32> oo(3 * nrays), nn(3 * nrays);
    for (size_t r = 0; r < nrays; ++r) {
        oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
        nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
    }
    d.check(vrt_hip_radiance_rays(d.ctx, nrays, oo.data(), 1, nn.data(), out ? &out[0].x : nullptr, image, pack_flags), "vrt_hip_radiance_rays");
}
// The same for rays and results that live on the device (3 floats per origin -- or 3 in all with origin_per_ray = false -- and
// per direction, 4 floats of radiance and / or one u32 per ray): enqueued on hip_stream, nothing waits.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const gaussians_t &gaussians,
                          f32 *d_radiance, u32 *d_image, int pack_flags, void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    d.check(vrt_hip_radiance_rays_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, d_radiance, d_image, pack_flags, hip_stream),
            "vrt_hip_radiance_rays_device");
}
// Gradient bundles: given grad_radiance[r] = d(loss) / d(out[r] of radiance_rays) for the same rays, the derivative of the loss with
// respect to the Gaussians (vrt_hip_radiance_rays_grad in include/vrt_hip.h has the function, the fixed kept lists and the supported
// pairs: {vcl, libm} x {abramowitz_stegun, libm}; any other pair throws).  grad_out: gaussians.size() rows of VRT_HIP_GRAD_STRIDE
// floats, OVERWRITTEN: [0..3] d albedo, [4..6] d mu, [7] d sigma, [8] d magnitude, [9..11] 0.  Summed with float atomics on the
// device: not bitwise reproducible.  grad_rays_out (the overload with it; either output nullable, not both): nrays rows of
// VRT_HIP_RAY_GRAD_STRIDE floats, [0..2] d(loss) / d(origin), [3] 0, [4..6] the tangential d(loss) / d(direction), [7] 0 -- summed without
// atomics, bitwise reproducible ("ray gradients" in include/vrt_hip.h).  Each ray's kept list is held fixed.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_grad(const vec4f_t *o, const vec4f_t *n, size_t nrays, const gaussians_t &gaussians, const vec4f_t *grad_radiance, f32 *grad_out,
                        f32 *grad_rays_out)
{
    static_assert(sizeof(vec4f_t) == 4 * sizeof(f32), "grad_radiance is handed to the library as 4 floats per ray");
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    std::vector<f32> oo(3 * nrays), nn(3 * nrays);
    for (size_t r = 0; r < nrays; ++r) {
        oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
        nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
    }
    d.check(vrt_hip_radiance_rays_grad_rays(d.ctx, nrays, oo.data(), 1, nn.data(), grad_radiance ? &grad_radiance[0].x : nullptr, grad_out, grad_rays_out),
            "vrt_hip_radiance_rays_grad_rays");
}
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_grad(const vec4f_t *o, const vec4f_t *n, size_t nrays, const gaussians_t &gaussians, const vec4f_t *grad_radiance, f32 *grad_out)
{
    radiance_rays_grad<Exp, Erf>(o, n, nrays, gaussians, grad_radiance, grad_out, nullptr);
}
// The same on the device: ADDS into d_grad (the caller clears it), STORES d_grad_rays (16-byte aligned), enqueued on hip_stream, nothing
// waits.  Without d_grad no atomic add is issued.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_grad_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const gaussians_t &gaussians,
                               const f32 *d_grad_radiance, f32 *d_grad, f32 *d_grad_rays, void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    d.check(vrt_hip_radiance_rays_grad_rays_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, d_grad_radiance, d_grad, d_grad_rays, hip_stream),
            "vrt_hip_radiance_rays_grad_rays_device");
}
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_grad_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const gaussians_t &gaussians,
                               const f32 *d_grad_radiance, f32 *d_grad, void *hip_stream)
{
    radiance_rays_grad_device<Exp, Erf>(d_origins, origin_per_ray, d_dirs, nrays, gaussians, d_grad_radiance, d_grad, nullptr, hip_stream);
}
// Tangent bundles: forward mode, J . v.  Given a direction in parameter space -- tangent (nullable): gaussians.size() rows of
// VRT_HIP_GRAD_STRIDE floats in radiance_rays_grad's layout, [0..3] d albedo, [4..6] d mu, [7] d sigma, [8] d magnitude, [9..11] never read;
// ray_tangent (nullable, not both): nrays rows of VRT_HIP_RAY_GRAD_STRIDE floats, [0..2] d origin, [4..6] d direction (only its part
// perpendicular to the direction counts), [3] and [7] never read -- out[r] is how out[r] of radiance_rays moves along it, each ray's kept
// list held fixed (vrt_hip_radiance_rays_tangent in include/vrt_hip.h; the pairs of radiance_rays_grad, any other throws).  Stored, no
// atomic add: bitwise reproducible.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_tangent(const vec4f_t *o, const vec4f_t *n, size_t nrays, const gaussians_t &gaussians, const f32 *tangent, const f32 *ray_tangent,
                           vec4f_t *out)
{
    static_assert(sizeof(vec4f_t) == 4 * sizeof(f32), "out is handed to the library as 4 floats per ray");
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    std::vector<f32> oo(3 * nrays), nn(3 * nrays);
    for (size_t r = 0; r < nrays; ++r) {
        oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
        nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
    }
    d.check(vrt_hip_radiance_rays_tangent(d.ctx, nrays, oo.data(), 1, nn.data(), tangent, ray_tangent, out ? &out[0].x : nullptr),
            "vrt_hip_radiance_rays_tangent");
}
// The same on the device (all three 16-byte aligned): STORES d_out, enqueued on hip_stream, nothing waits.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_tangent_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const gaussians_t &gaussians,
                                  const f32 *d_tangent, const f32 *d_ray_tangent, f32 *d_out, void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    d.check(vrt_hip_radiance_rays_tangent_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, d_tangent, d_ray_tangent, d_out, hip_stream),
            "vrt_hip_radiance_rays_tangent_device");
}
// Gauss-Newton diagonal bundles: diag(J^T W J) of radiance_rays for the same rays -- per parameter the sum over rays and channels of
// weights[r] (nullable: all 1) times the squared derivative of that channel of that ray, each ray's kept list held fixed
// (vrt_hip_radiance_rays_gn_diag in include/vrt_hip.h; the pairs of radiance_rays_grad, any other throws).  diag_out: gaussians.size() rows
// of VRT_HIP_GRAD_STRIDE floats in radiance_rays_grad's layout, OVERWRITTEN, [9..11] 0.  Float atomics on the device: not bitwise
// reproducible unless vrt_hip_set_grad_ordered is on.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_gn_diag(const vec4f_t *o, const vec4f_t *n, size_t nrays, const gaussians_t &gaussians, const vec4f_t *weights, f32 *diag_out)
{
    static_assert(sizeof(vec4f_t) == 4 * sizeof(f32), "weights are handed to the library as 4 floats per ray");
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    std::vector<f32> oo(3 * nrays), nn(3 * nrays);
    for (size_t r = 0; r < nrays; ++r) {
        oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
        nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
    }
    d.check(vrt_hip_radiance_rays_gn_diag(d.ctx, nrays, oo.data(), 1, nn.data(), weights ? &weights[0].x : nullptr, diag_out), "vrt_hip_radiance_rays_gn_diag");
}
// The same on the device (d_weights 16-byte aligned, nullable): ADDS into d_diag (the caller clears it), enqueued on hip_stream, nothing waits.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void radiance_rays_gn_diag_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const gaussians_t &gaussians,
                                  const f32 *d_weights, f32 *d_diag, void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    d.check(vrt_hip_radiance_rays_gn_diag_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, d_weights, d_diag, hip_stream),
            "vrt_hip_radiance_rays_gn_diag_device");
}
// Transmittance bundles: broadcast_transmittance for ANY number of rays at ns depths each in ONE call, under the same per-ray cull
// (vrt_hip_transmittance_bundle in include/vrt_hip.h: the exponent moves by less than 0.8 * cull_eps * min(N, 4096) = 3.3e-6 at the
// defaults).  s: ns sample distances shared by all rays (s_per_ray = false) or nrays * ns, [r * ns + k]; T_out[r * ns + k].  Shadow
// rays are ns = 1; a depth profile along a ray is one call.  vrt::broadcast_transmittance above stays the reference's full sum.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void transmittance_bundle(const vec4f_t *o, const vec4f_t *n, size_t nrays, const f32 *s, size_t ns, bool s_per_ray, const gaussians_t &gaussians,
                          f32 *T_out)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    std::vector<f32> oo(3 * nrays), nn(3 * nrays);
    for (size_t r = 0; r < nrays; ++r) {
        oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
        nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
    }
    d.check(vrt_hip_transmittance_bundle(d.ctx, nrays, oo.data(), 1, nn.data(), s, ns, s_per_ray ? 1 : 0, T_out), "vrt_hip_transmittance_bundle");
}
// The same for rays, samples and results that live on the device: enqueued on hip_stream, nothing waits.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void transmittance_bundle_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const f32 *d_s, size_t ns, bool s_per_ray,
                                 const gaussians_t &gaussians, f32 *d_T, void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    d.check(vrt_hip_transmittance_bundle_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, d_s, ns, s_per_ray ? 1 : 0, d_T, hip_stream),
            "vrt_hip_transmittance_bundle_device");
}
// Depth bundles: the distance along ANY number of rays at which their transmittance falls to nt levels each, in ONE call under the same
// per-ray cull (vrt_hip_depth_bundle in include/vrt_hip.h): depth_out[r * nt + k] is 0 where ray r starts at or below the level, +inf
// where it never gets there, and otherwise the upper end of a bracket around the crossing no wider than max(ulp, s_end * 2^-24) --
// transmittance_bundle at that depth returns a T <= tau.  tau: nt levels shared by all rays (tau_per_ray = false) or nrays * nt,
// [r * nt + k].  tau = 0.5 is a median-depth map; a first hit to start shadow rays from is one call (host/first_hit_example.cpp).
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void depth_bundle(const vec4f_t *o, const vec4f_t *n, size_t nrays, const f32 *tau, size_t nt, bool tau_per_ray, const gaussians_t &gaussians,
                  f32 *depth_out)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    std::vector<f32> oo(3 * nrays), nn(3 * nrays);
    for (size_t r = 0; r < nrays; ++r) {
        oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
        nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
    }
    d.check(vrt_hip_depth_bundle(d.ctx, nrays, oo.data(), 1, nn.data(), tau, nt, tau_per_ray ? 1 : 0, depth_out), "vrt_hip_depth_bundle");
}
// The same for rays, levels and results that live on the device: enqueued on hip_stream, nothing waits.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void depth_bundle_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const f32 *d_tau, size_t nt, bool tau_per_ray,
                         const gaussians_t &gaussians, f32 *d_depth, void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    d.check(vrt_hip_depth_bundle_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, d_tau, nt, tau_per_ray ? 1 : 0, d_depth, hip_stream),
            "vrt_hip_depth_bundle_device");
}
// Transmittance gradient bundles: given grad_T[r * ns + k] = d(loss) / d(T_out[r * ns + k] of transmittance_bundle) for the same rays and
// samples (wrt = VRT_HIP_TGRAD_T) -- or d(loss) / d(depth_out[r * ns + k] of depth_bundle), with s the depths it returned, s_per_ray = true
// (wrt = VRT_HIP_TGRAD_DEPTH: the derivative of the ideal crossing; a depth of +inf, 0 or NaN contributes nothing) -- the derivative of the
// loss with respect to the Gaussians and to the samples or levels (vrt_hip_transmittance_bundle_grad in include/vrt_hip.h has the
// function, the fixed kept lists and the supported pairs, those of radiance_rays_grad).  grad_out (nullable): gaussians.size() rows of
// VRT_HIP_GRAD_STRIDE floats, OVERWRITTEN: [4..6] d mu, [7] d sigma, [8] d magnitude, everything else 0.  grad_s_out (nullable): nrays *
// ns, d(loss) / d(s) or d(loss) / d(tau).  A sample with grad_T == 0 is skipped exactly.  The table is not bitwise reproducible.
// grad_rays_out (the overload with it; nullable): the ray rows, as radiance_rays_grad's, which are.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void transmittance_bundle_grad(const vec4f_t *o, const vec4f_t *n, size_t nrays, const f32 *s, size_t ns, bool s_per_ray, const gaussians_t &gaussians,
                               const f32 *grad_T, int wrt, f32 *grad_out, f32 *grad_s_out, f32 *grad_rays_out)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    std::vector<f32> oo(3 * nrays), nn(3 * nrays);
    for (size_t r = 0; r < nrays; ++r) {
        oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
        nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
    }
    d.check(vrt_hip_transmittance_bundle_grad_rays(d.ctx, nrays, oo.data(), 1, nn.data(), s, ns, s_per_ray ? 1 : 0, grad_T, wrt, grad_out, grad_s_out,
                                                   grad_rays_out),
            "vrt_hip_transmittance_bundle_grad_rays");
}
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void transmittance_bundle_grad(const vec4f_t *o, const vec4f_t *n, size_t nrays, const f32 *s, size_t ns, bool s_per_ray, const gaussians_t &gaussians,
                               const f32 *grad_T, int wrt, f32 *grad_out, f32 *grad_s_out)
{
    transmittance_bundle_grad<Exp, Erf>(o, n, nrays, s, ns, s_per_ray, gaussians, grad_T, wrt, grad_out, grad_s_out, nullptr);
}
// The same on the device: ADDS into d_grad (the caller clears it), STORES d_grad_s and d_grad_rays, enqueued on hip_stream, nothing waits.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void transmittance_bundle_grad_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const f32 *d_s, size_t ns, bool s_per_ray,
                                      const gaussians_t &gaussians, const f32 *d_grad_T, int wrt, f32 *d_grad, f32 *d_grad_s, f32 *d_grad_rays,
                                      void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    d.check(vrt_hip_transmittance_bundle_grad_rays_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, d_s, ns, s_per_ray ? 1 : 0, d_grad_T, wrt,
                                                          d_grad, d_grad_s, d_grad_rays, hip_stream),
            "vrt_hip_transmittance_bundle_grad_rays_device");
}
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void transmittance_bundle_grad_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const f32 *d_s, size_t ns, bool s_per_ray,
                                      const gaussians_t &gaussians, const f32 *d_grad_T, int wrt, f32 *d_grad, f32 *d_grad_s, void *hip_stream)
{
    transmittance_bundle_grad_device<Exp, Erf>(d_origins, origin_per_ray, d_dirs, nrays, d_s, ns, s_per_ray, gaussians, d_grad_T, wrt, d_grad, d_grad_s, nullptr,
                                               hip_stream);
}
// Transmittance tangent bundles: forward mode, J . v of transmittance_bundle (wrt = VRT_HIP_TGRAD_T, at the samples s) or of depth_bundle
// (VRT_HIP_TGRAD_DEPTH, s = the nrays * ns depths it returned, s_per_ray = true) along a direction: tangent (nullable; rows as
// radiance_rays_tangent's, [4..8] read), ray_tangent (nullable; as radiance_rays_tangent's) and s_tangent (nullable; d s or d tau, nrays * ns
// or, with s_tangent_per_ray = false, ns), not all three null.  out[r * ns + k], stored, no atomic add: bitwise reproducible
// (vrt_hip_transmittance_bundle_tangent in include/vrt_hip.h; the pairs of radiance_rays_grad, any other throws).
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void transmittance_bundle_tangent(const vec4f_t *o, const vec4f_t *n, size_t nrays, const f32 *s, size_t ns, bool s_per_ray, const gaussians_t &gaussians,
                                  int wrt, const f32 *tangent, const f32 *ray_tangent, const f32 *s_tangent, bool s_tangent_per_ray, f32 *out)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    std::vector<f32> oo(3 * nrays), nn(3 * nrays);
    for (size_t r = 0; r < nrays; ++r) {
        oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
        nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
    }
    d.check(vrt_hip_transmittance_bundle_tangent(d.ctx, nrays, oo.data(), 1, nn.data(), s, ns, s_per_ray ? 1 : 0, wrt, tangent, ray_tangent, s_tangent,
                                                 s_tangent_per_ray ? 1 : 0, out),
            "vrt_hip_transmittance_bundle_tangent");
}
// The same on the device (d_tangent and d_ray_tangent 16-byte aligned): STORES d_out, enqueued on hip_stream, nothing waits.
template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
void transmittance_bundle_tangent_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const f32 *d_s, size_t ns,
                                         bool s_per_ray, const gaussians_t &gaussians, int wrt, const f32 *d_tangent, const f32 *d_ray_tangent,
                                         const f32 *d_s_tangent, bool s_tangent_per_ray, f32 *d_out, void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians.gaussians);
    d.options(Exp, Erf);
    d.check(vrt_hip_transmittance_bundle_tangent_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, d_s, ns, s_per_ray ? 1 : 0, wrt, d_tangent,
                                                        d_ray_tangent, d_s_tangent, s_tangent_per_ray ? 1 : 0, d_out, hip_stream),
            "vrt_hip_transmittance_bundle_tangent_device");
}
// Ray bundles cull through the Morton index of the scene from the next call on (vrt_hip_set_ray_index in include/vrt_hip.h: off by
// default, the same radiance and the same pixels bit for bit either way; the index is made once per scene).
inline void set_ray_index(bool on)
{
    auto &d = detail::device_t::get();
    d.check(vrt_hip_set_ray_index(d.ctx, on ? 1 : 0), "vrt_hip_set_ray_index");
}
// Ray bundles of more than 64 rays are shaded in an order that puts rays which keep the same bounding spheres into the same wave, from
// the next call on (vrt_hip_set_ray_sort in include/vrt_hip.h: off by default; every result stays at the caller's ray index, the same
// bits either way; for probes, second bounces, shuffled batches -- a camera's own order gains nothing).
inline void set_ray_sort(bool on)
{
    auto &d = detail::device_t::get();
    d.check(vrt_hip_set_ray_sort(d.ctx, on ? 1 : 0), "vrt_hip_set_ray_sort");
}
// Gradient bundles build their table without float atomics from the next call on: bit for bit reproducible, summed in a documented
// order (vrt_hip_set_grad_ordered in include/vrt_hip.h: off by default; an ordered call waits once for its stream).
inline void set_grad_ordered(bool on)
{
    auto &d = detail::device_t::get();
    d.check(vrt_hip_set_grad_ordered(d.ctx, on ? 1 : 0), "vrt_hip_set_grad_ordered");
}
// The records the last ordered gradient bundle reduced its table from, in consumed order (vrt_hip_get_grad_records): record i is
// rows[9 * i .. 9 * i + 8] = columns 0..8 of the table, the share of ray[i] in the row of Gaussian gauss[i].  Waits for the call.
struct grad_records_t {
    std::vector<u32> gauss, ray;
    std::vector<f32> rows;
};
inline grad_records_t grad_records()
{
    auto &d = detail::device_t::get();
    grad_records_t out;
    size_t n = 0;
    const int rc = vrt_hip_get_grad_records(d.ctx, nullptr, nullptr, nullptr, 0, &n);
    if (n == 0) { d.check(rc, "vrt_hip_get_grad_records"); return out; }
    out.gauss.resize(n); out.ray.resize(n); out.rows.resize(n * 9);
    d.check(vrt_hip_get_grad_records(d.ctx, out.gauss.data(), out.ray.data(), out.rows.data(), n, &n), "vrt_hip_get_grad_records");
    return out;
}
// Ray plans: the cull of a bundle run ONCE and kept on the device ("Ray plans" in include/vrt_hip.h).  While a plan is bound
// (vrt::set_ray_plan) every bundle call above with the plan's number of rays takes each ray's kept list from it -- the same bits, no
// sphere test, no member test, no sort, no count pass: for loops that send the same rays through the same scene many times (a CG solve on
// J and J^T, a forward and its backward).  Strict by default: a call after the scene or the cull options changed throws; with
// keep_lists the lists stay in force across scene updates of the same size, which is the function the gradient and tangent bundles
// differentiate.  An RAII handle of the process-wide context: movable, not copyable; its destructor unbinds and frees the plan.
class ray_plan {
  public:
    ray_plan() = default;
    // from host rays, one origin per ray (as the bundle calls take them); the scene and the pair as the bundle calls set them
    template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
    static ray_plan make(const vec4f_t *o, const vec4f_t *n, size_t nrays, const gaussians_t &gaussians)
    {
        auto &d = detail::device_t::get();
        d.upload_scene(gaussians.gaussians);
        d.options(Exp, Erf);
        std::vector<f32> oo(3 * nrays), nn(3 * nrays);
        for (size_t r = 0; r < nrays; ++r) {
            oo[3 * r] = o[r].x; oo[3 * r + 1] = o[r].y; oo[3 * r + 2] = o[r].z;
            nn[3 * r] = n[r].x; nn[3 * r + 1] = n[r].y; nn[3 * r + 2] = n[r].z;
        }
        ray_plan p;
        d.check(vrt_hip_ray_plan_create(d.ctx, nrays, oo.data(), 1, nn.data(), &p.plan_), "vrt_hip_ray_plan_create");
        return p;
    }
    // from rays on the device: enqueued on hip_stream and waited for; the plan is complete and usable on any stream
    template <exp_kind Exp = exp_kind::vcl, erf_kind Erf = erf_kind::abramowitz_stegun>
    static ray_plan make_device(const f32 *d_origins, bool origin_per_ray, const f32 *d_dirs, size_t nrays, const gaussians_t &gaussians, void *hip_stream)
    {
        auto &d = detail::device_t::get();
        d.upload_scene(gaussians.gaussians);
        d.options(Exp, Erf);
        ray_plan p;
        d.check(vrt_hip_ray_plan_create_device(d.ctx, nrays, d_origins, origin_per_ray ? 1 : 0, d_dirs, hip_stream, &p.plan_), "vrt_hip_ray_plan_create_device");
        return p;
    }
    ray_plan(const ray_plan &) = delete;
    ray_plan &operator=(const ray_plan &) = delete;
    ray_plan(ray_plan &&o) noexcept : plan_(o.plan_) { o.plan_ = nullptr; }
    ray_plan &operator=(ray_plan &&o) noexcept
    {
        if (this != &o) { reset(); plan_ = o.plan_; o.plan_ = nullptr; }
        return *this;
    }
    ~ray_plan() { reset(); }
    void reset() noexcept // waits for bundles in flight; the bound plan is unbound first
    {
        if (plan_) (void)vrt_hip_ray_plan_destroy(detail::device_t::get().ctx, plan_);
        plan_ = nullptr;
    }
    explicit operator bool() const { return plan_ != nullptr; }
    vrt_hip_ray_plan *get() const { return plan_; }
    vrt_hip_ray_plan_info info() const
    {
        auto &d = detail::device_t::get();
        vrt_hip_ray_plan_info i{};
        d.check(vrt_hip_get_ray_plan_info(d.ctx, plan_, &i), "vrt_hip_get_ray_plan_info");
        return i;
    }

  private:
    vrt_hip_ray_plan *plan_ = nullptr;
};
// Binds `plan` for every later bundle call; vrt::clear_ray_plan() binds none.  Waits for bundles in flight.
inline void set_ray_plan(const ray_plan &plan, bool keep_lists = false)
{
    auto &d = detail::device_t::get();
    d.check(vrt_hip_set_ray_plan(d.ctx, plan.get(), plan.get() && keep_lists ? VRT_HIP_PLAN_KEEP_LISTS : 0), "vrt_hip_set_ray_plan");
}
inline void clear_ray_plan()
{
    auto &d = detail::device_t::get();
    d.check(vrt_hip_set_ray_plan(d.ctx, nullptr, 0), "vrt_hip_set_ray_plan");
}
// The plan's lists read back: ray r (the caller's index) keeps entries[offsets[r] .. offsets[r + 1]), scene indices in ascending order.
struct ray_plan_lists_t {
    std::vector<u64> offsets; // nrays + 1
    std::vector<u32> entries;
};
inline ray_plan_lists_t ray_plan_lists(const ray_plan &plan)
{
    auto &d = detail::device_t::get();
    const vrt_hip_ray_plan_info i = plan.info();
    ray_plan_lists_t out;
    out.offsets.resize(i.rays + 1);
    out.entries.resize(i.entries);
    static_assert(sizeof(u64) == sizeof(uint64_t), "the offsets are read as they stand");
    d.check(vrt_hip_get_ray_plan_lists(d.ctx, plan.get(), reinterpret_cast<uint64_t *>(out.offsets.data()), out.entries.empty() ? nullptr : out.entries.data()),
            "vrt_hip_get_ray_plan_lists");
    return out;
}
// The scene from DEVICE memory (vrt_hip_set_gaussians_device in include/vrt_hip.h): d_mu [n, 3], d_albedo [n, 4] with alpha in column 3,
// d_sigma [n], d_magnitude [n], float32; everything enqueued on hip_stream, nothing waited for (but where a buffer has to grow), the same
// scene bit for bit as the same values uploaded from the host.  It stays the scene of every later call that is given an EMPTY
// gaussians_t; a call with Gaussians of its own uploads those, as always.  Tile sets of the scene before are gone.
inline void set_gaussians_device(size_t n, const f32 *d_mu, const f32 *d_albedo, const f32 *d_sigma, const f32 *d_magnitude, void *hip_stream)
{
    auto &d = detail::device_t::get();
    d.check(vrt_hip_set_gaussians_device(d.ctx, n, d_mu, d_albedo, d_sigma, d_magnitude, hip_stream), "vrt_hip_set_gaussians_device");
    d.device_scene = true;
    d.scene_key = nullptr;
    ++d.generation;
}
// ======== end of the extension ==========================================================================================

// ---- rt.cpp:8-27 -----------------------------------------------------------------------------------------------------
// transmittance_step passes on, like its siblings (detail::device_t::check), the error of vrt_hip_transmittance_step, which refuses the
// arguments with which the reference's loop `t <= s; t += delta` does not end or runs for long: s = +inf, s >= delta * 2^23, a delta
// that is no normal positive float, more than 2^23 density evaluations (include/vrt_hip.h).
inline f32 transmittance_step(const vec4f_t o, const vec4f_t n, const f32 s, const f32 delta, const std::vector<gaussian_t> gaussians)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians);
    const f32 oo[3] = { o.x, o.y, o.z }, nn[3] = { n.x, n.y, n.z };
    f32 T = 0.f;
    d.check(vrt_hip_transmittance_step(d.ctx, oo, nn, &s, 1, delta, &T), "vrt_hip_transmittance_step");
    return T;
}
inline f32 density(const vec4f_t pt, const std::vector<gaussian_t> gaussians)
{
    auto &d = detail::device_t::get();
    d.upload_scene(gaussians);
    const f32 p[3] = { pt.x, pt.y, pt.z };
    f32 D = 0.f;
    d.check(vrt_hip_density(d.ctx, 1, p, &D), "vrt_hip_density");
    return D;
}

} // namespace vrt

// ---- gaussians-from-file.h:5 / .cpp:7-44: every "v x y z" line of an OBJ file becomes a Gaussian -----------------------
inline std::vector<vrt::gaussian_t> read_from_obj(const char *const filename)
{
    FILE *f = std::fopen(filename, "r");
    if (!f) {
        std::fprintf(stderr, "[ ERROR ]\tread_from_obj: cannot open %s\n", filename);
        std::exit(EXIT_FAILURE); // the reference exits too (gaussians-from-file.cpp:16)
    }
    std::vector<std::array<f32, 3>> verts;
    char line[1024];
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] != 'v' || (line[1] != ' ' && line[1] != '\t')) continue;
        char *p = line + 1;
        std::array<f32, 3> v{};
        for (int c = 0; c < 3; ++c) v[c] = (f32)std::strtod(p, &p);
        verts.push_back(v);
    }
    std::fclose(f);
    const f32 sig = verts.size() < 300 ? 0.3f : verts.size() < 1000 ? 0.15f : 0.05f;
    std::vector<vrt::gaussian_t> g;
    g.reserve(verts.size());
    for (const auto &v : verts) {
        vrt::vec4f_t pt{ v[0], v[1], v[2], 0.0f };
        vrt::vec4f_t c = pt;
        c.normalize();
        g.push_back(vrt::gaussian_t{ c * 0.5f + vrt::vec4f_t{ 0.5f, 0.5f, 0.5f, 1.0f }, pt, sig, 1.0f });
    }
    return g;
}
