// shadow_rays_example.cpp -- radiance and a depth profile of the same rays (the extensions of include/vrt/vrt.hpp): a small bundle is
// shaded with vrt::radiance_rays, then vrt::transmittance_bundle gives T at 8 depths along every one of them -- what a caller asks
// after a first hit: how much of a light behind depth s reaches the eye along this ray.
// Prints one line per ray: "ray <r> o <3 floats> n <3 floats> L <4 floats> T <8 floats>", every float with 9 significant digits (a
// float32 survives that), depths 0.5, 1.5, ... 7.5.
#include <cstdio>

#include "../../include/vrt/vrt.hpp"

using namespace vrt;

int main()
{
    const gaussians_t scene{ { gaussian_t{ { 0.f, 1.f, 0.f, .1f }, { .3f, .3f, .5f }, 0.1f, 2.f },
                               gaussian_t{ { 0.f, 0.f, 1.f, .7f }, { -.3f, -.3f, 0.f }, 0.4f, .7f },
                               gaussian_t{ { 1.f, 0.f, 0.f, 1.f }, { 0.f, 0.f, 2.f }, .75f, 1.f } } };
    constexpr u32 w = 4, h = 3, ns = 8;
    const vec4f_t eye{ 0.1f, -0.05f, -4.f };
    std::vector<vec4f_t> o(w * h), n(w * h), L(w * h);
    for (u32 i = 0; i < h; ++i)
        for (u32 j = 0; j < w; ++j) {
            vec4f_t d = vec4f_t{ -0.6f + 1.2f * (j + 0.5f) / w, -0.6f + 1.2f * (i + 0.5f) / h, 0.5f } - eye;
            d.normalize();
            o[i * w + j] = eye; n[i * w + j] = d;
        }
    f32 s[ns];
    for (u32 k = 0; k < ns; ++k) s[k] = 0.5f + (f32)k;
    std::vector<f32> T(o.size() * ns);
    radiance_rays(o.data(), n.data(), o.size(), scene, L.data());
    transmittance_bundle(o.data(), n.data(), o.size(), s, ns, false, scene, T.data());
    for (size_t r = 0; r < o.size(); ++r) {
        std::printf("ray %zu o %.9g %.9g %.9g n %.9g %.9g %.9g L %.9g %.9g %.9g %.9g T", r, o[r].x, o[r].y, o[r].z, n[r].x, n[r].y, n[r].z, L[r].x,
                    L[r].y, L[r].z, L[r].w);
        for (u32 k = 0; k < ns; ++k) std::printf(" %.9g", T[r * ns + k]);
        std::printf("\n");
    }
    return 0;
}
