// ray_plan_example.cpp -- the inner loop of a Gauss-Newton step on a ray plan (the extension of include/vrt/vrt.hpp): ONE plan for the rays
// of a small pinhole, then k rounds of a tangent bundle (J v) and a gradient bundle (J^T of what came back) over it, as conjugate
// gradients on J^T J issues them -- none of which culls again.  Prints the plan's info and, per round, |J v|^2 and <v, J^T J v>, which
// are one number (the adjoint identity); the first round is run unplanned as well and must give the same bits, or exit status 2.
// vrt::set_grad_ordered makes the tables reproducible, so that the comparison is one of bits.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vrt/vrt.hpp"

using namespace vrt;

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 4;
    const gaussians_t scene{ { gaussian_t{ { 0.f, 1.f, 0.f, .1f }, { .3f, .3f, .5f }, 0.1f, 2.f },
                               gaussian_t{ { 0.f, 0.f, 1.f, .7f }, { -.3f, -.3f, 0.f }, 0.4f, .7f },
                               gaussian_t{ { 1.f, 0.f, 0.f, 1.f }, { 0.f, 0.f, 2.f }, .75f, 1.f } } };
    const size_t N = scene.gaussians.size();
    const u32 w = 16, h = 16;
    const vec4f_t eye{ 0.f, 0.f, -4.f };
    std::vector<vec4f_t> o(w * h, eye), n(w * h);
    for (u32 i = 0; i < h; ++i)
        for (u32 j = 0; j < w; ++j) {
            vec4f_t d = vec4f_t{ -0.5f + (j + 0.5f) / w, -0.5f + (i + 0.5f) / h, -3.f } - eye;
            d.normalize();
            n[i * w + j] = d;
        }
    const size_t nrays = n.size();
    // v: a direction in the Gaussians (rows of VRT_HIP_GRAD_STRIDE floats: d albedo, d mu, d sigma, d magnitude)
    std::vector<f32> v(N * VRT_HIP_GRAD_STRIDE, 0.f), JtJv(N * VRT_HIP_GRAD_STRIDE), first(N * VRT_HIP_GRAD_STRIDE);
    for (size_t j = 0; j < N; ++j)
        for (int c = 0; c < 9; ++c) v[j * VRT_HIP_GRAD_STRIDE + c] = 0.1f * std::sin(1.f + 3.f * j + c);
    std::vector<vec4f_t> Jv(nrays), Jv_first(nrays);

    set_grad_ordered(true);
    auto round = [&](std::vector<vec4f_t> &jv, std::vector<f32> &jtjv) {
        radiance_rays_tangent(o.data(), n.data(), nrays, scene, v.data(), nullptr, jv.data());
        radiance_rays_grad(o.data(), n.data(), nrays, scene, jv.data(), jtjv.data());
    };
    round(Jv_first, first); // unplanned: every call culls

    ray_plan plan = ray_plan::make(o.data(), n.data(), nrays, scene);
    const vrt_hip_ray_plan_info info = plan.info();
    std::printf("plan: %llu rays, %llu entries, %llu short, %llu long, longest list %llu, %llu bytes, sorted %llu, indexed %llu\n",
                (unsigned long long)info.rays, (unsigned long long)info.entries, (unsigned long long)info.short_rays, (unsigned long long)info.long_rays,
                (unsigned long long)info.longest, (unsigned long long)info.bytes, (unsigned long long)info.sorted, (unsigned long long)info.indexed);
    const ray_plan_lists_t lists = ray_plan_lists(plan);
    if (lists.offsets.size() != nrays + 1 || lists.offsets.back() != info.entries) return 2;

    set_ray_plan(plan);
    bool same = true;
    for (int k = 0; k < rounds; ++k) {
        round(Jv, JtJv);
        double jv2 = 0.0, vJtJv = 0.0;
        for (size_t r = 0; r < nrays; ++r) jv2 += (double)Jv[r].x * Jv[r].x + (double)Jv[r].y * Jv[r].y + (double)Jv[r].z * Jv[r].z + (double)Jv[r].w * Jv[r].w;
        for (size_t i = 0; i < v.size(); ++i) vJtJv += (double)v[i] * JtJv[i];
        std::printf("round %d: |J v|^2 %.9g  <v, J^T J v> %.9g\n", k, jv2, vJtJv);
        if (k == 0)
            same = !std::memcmp(Jv.data(), Jv_first.data(), nrays * sizeof(vec4f_t)) && !std::memcmp(JtJv.data(), first.data(), JtJv.size() * sizeof(f32));
        // the next direction: what a CG step would take from the residual; here simply the normalised J^T J v
        double norm = 0.0;
        for (f32 x : JtJv) norm += (double)x * x;
        norm = std::sqrt(norm);
        if (norm > 0.0)
            for (size_t i = 0; i < v.size(); ++i) v[i] = (f32)(JtJv[i] / norm);
    }
    clear_ray_plan();
    std::fprintf(stderr, "planned against unplanned: %s\n", same ? "identical" : "DIFFERENT");
    return same ? 0 : 2;
}
