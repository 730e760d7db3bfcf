// ray_bundle_example.cpp -- a stereo pair in ONE call of vrt::radiance_rays (the extension of include/vrt/vrt.hpp): the rays of
// two pinhole eyes, interleaved, each ray with its own origin.  Prints a checksum per eye; with a file name as argument it
// also writes the rays (origin, direction: 6 floats per ray) there, so that anyone can shade the same rays again.
// A second call shades the same rays through the Morton index of the scene (vrt::set_ray_index): the same bits, or exit status 2.
#include <cstdio>
#include <cstring>

#include "../../include/vrt/vrt.hpp"

using namespace vrt;

int main(int argc, char **argv)
{
    const gaussians_t scene{ { gaussian_t{ { 0.f, 1.f, 0.f, .1f }, { .3f, .3f, .5f }, 0.1f, 2.f },
                               gaussian_t{ { 0.f, 0.f, 1.f, .7f }, { -.3f, -.3f, 0.f }, 0.4f, .7f },
                               gaussian_t{ { 1.f, 0.f, 0.f, 1.f }, { 0.f, 0.f, 2.f }, .75f, 1.f } } };
    const u32 w = 16, h = 16;
    const vec4f_t eye[2] = { { -0.1f, 0.f, -4.f }, { 0.1f, 0.f, -4.f } };
    std::vector<vec4f_t> o(2 * w * h), n(2 * w * h), L(2 * w * h);
    std::vector<u32> px(2 * w * h);
    for (u32 i = 0; i < h; ++i)
        for (u32 j = 0; j < w; ++j)
            for (u32 e = 0; e < 2; ++e) { // ray 2 * pixel + eye: both eyes look at the plane z = -3 in front of their midpoint
                const size_t r = 2 * (size_t)(i * w + j) + e;
                vec4f_t d = vec4f_t{ -0.5f + (j + 0.5f) / w, -0.5f + (i + 0.5f) / h, -3.f } - eye[e];
                d.normalize();
                o[r] = eye[e]; n[r] = d;
            }
    radiance_rays(o.data(), n.data(), o.size(), scene, L.data(), px.data());
    for (u32 e = 0; e < 2; ++e) {
        double sum = 0.0;
        u32 hash = 0;
        for (size_t r = e; r < L.size(); r += 2) {
            sum += (double)L[r].x + (double)L[r].y + (double)L[r].z + (double)L[r].w;
            hash = hash * 31u + px[r];
        }
        std::printf("%s eye: radiance sum %.9g pixel hash %08x\n", e ? "right" : "left", sum, hash);
    }
    std::vector<vec4f_t> L2(L.size());
    std::vector<u32> px2(px.size());
    set_ray_index(true);
    radiance_rays(o.data(), n.data(), o.size(), scene, L2.data(), px2.data());
    const bool same = !std::memcmp(L.data(), L2.data(), L.size() * sizeof(vec4f_t)) && !std::memcmp(px.data(), px2.data(), px.size() * sizeof(u32));
    std::fprintf(stderr, "ray index: %s\n", same ? "identical" : "DIFFERENT");
    if (!same) return 2;
    if (argc > 1) {
        FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 1;
        for (size_t r = 0; r < o.size(); ++r) {
            const f32 row[6] = { o[r].x, o[r].y, o[r].z, n[r].x, n[r].y, n[r].z };
            std::fwrite(row, sizeof row, 1, f);
        }
        std::fclose(f);
    }
    return 0;
}
