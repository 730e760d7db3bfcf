// first_hit_example.cpp -- a first hit and its shadow ray (the extensions of include/vrt/vrt.hpp): a small bundle is shaded with
// vrt::radiance_rays, vrt::depth_bundle gives the median depth of every ray (the distance at which its transmittance falls to 0.5; +inf
// where it never does), and from the points at those depths shadow rays go to a light: vrt::transmittance_bundle with one sample per
// ray, the distance to the light.
// Prints one line per ray: "ray <r> o <3 floats> n <3 floats> L <4 floats> depth <float>", and for a ray that has a hit
// " hit <3 floats> to_light <3 floats> dist <float> T <float>"; every float with 9 significant digits (a float32 survives that).
#include <cmath>
#include <cstdio>

#include "../../include/vrt/vrt.hpp"

using namespace vrt;

int main()
{
    const gaussians_t scene{ { gaussian_t{ { 0.f, 1.f, 0.f, .1f }, { .3f, .3f, .5f }, 0.1f, 2.f },
                               gaussian_t{ { 0.f, 0.f, 1.f, .7f }, { -.3f, -.3f, 0.f }, 0.4f, .7f },
                               gaussian_t{ { 1.f, 0.f, 0.f, 1.f }, { 0.f, 0.f, 2.f }, .75f, 1.f } } };
    constexpr u32 w = 4, h = 3;
    const vec4f_t eye{ 0.1f, -0.05f, -4.f }, light{ 3.f, 4.f, -1.f };
    std::vector<vec4f_t> o(w * h), n(w * h), L(w * h);
    for (u32 i = 0; i < h; ++i)
        for (u32 j = 0; j < w; ++j) {
            vec4f_t d = vec4f_t{ -0.9f + 1.8f * (j + 0.5f) / w, -0.9f + 1.8f * (i + 0.5f) / h, 0.5f } - eye;
            d.normalize();
            o[i * w + j] = eye; n[i * w + j] = d;
        }
    const f32 tau = 0.5f;
    std::vector<f32> depth(o.size());
    radiance_rays(o.data(), n.data(), o.size(), scene, L.data());
    depth_bundle(o.data(), n.data(), o.size(), &tau, 1, false, scene, depth.data());

    // shadow rays of the rays that have a hit
    std::vector<size_t> ray_of;
    std::vector<vec4f_t> so, sn;
    std::vector<f32> dist;
    for (size_t r = 0; r < o.size(); ++r) {
        if (!std::isfinite(depth[r])) continue;
        const vec4f_t hit = o[r] + n[r] * depth[r];
        vec4f_t d = light - hit;
        const f32 len = std::sqrt(d.sqnorm());
        d.normalize();
        ray_of.push_back(r); so.push_back(hit); sn.push_back(d); dist.push_back(len);
    }
    std::vector<f32> T(so.size());
    transmittance_bundle(so.data(), sn.data(), so.size(), dist.data(), 1, true, scene, T.data());

    size_t k = 0;
    for (size_t r = 0; r < o.size(); ++r) {
        std::printf("ray %zu o %.9g %.9g %.9g n %.9g %.9g %.9g L %.9g %.9g %.9g %.9g depth %.9g", r, o[r].x, o[r].y, o[r].z, n[r].x, n[r].y, n[r].z,
                    L[r].x, L[r].y, L[r].z, L[r].w, depth[r]);
        if (k < ray_of.size() && ray_of[k] == r) {
            std::printf(" hit %.9g %.9g %.9g to_light %.9g %.9g %.9g dist %.9g T %.9g", so[k].x, so[k].y, so[k].z, sn[k].x, sn[k].y, sn[k].z, dist[k], T[k]);
            ++k;
        }
        std::printf("\n");
    }
    return 0;
}
