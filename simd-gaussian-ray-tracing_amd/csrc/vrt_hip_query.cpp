// vrt_hip_query.cpp -- point queries of libvrt_hip.so: transmittance, density and radiance along caller-given rays or at
// caller-given points, and the Exp / Erf approximations evaluated on the device.
#include <initializer_list>

#include "vrt_hip_ctx.hpp"
#include "vrt_step_guard.hpp"

using namespace vrtk;

// The shape of every query: the host arrays `in` uploaded to device temporaries (freed on every way out), the scene tables
// brought up to date when the query reads them, launch(inputs, result) on the context's stream, `n_out` results read back.
template <typename Out, typename Launch>
static int query(vrt_hip_ctx *c, bool scene, std::initializer_list<std::pair<const float *, size_t>> in, size_t n_out, void *out,
                 Launch launch)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (scene) { int rc = rebuild_tables(c); if (rc) return rc; }
    DevBuf<float> d_in[3];
    DevBuf<Out> d_out;
    int k = 0;
    for (const auto &a : in) {
        HIPCHK(c, d_in[k].reserve(a.second));
        if (a.second) HIPCHK(c, hipMemcpy(d_in[k].p, a.first, a.second * 4, hipMemcpyHostToDevice));
        ++k;
    }
    HIPCHK(c, d_out.reserve(n_out));
    launch(d_in, d_out.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_out) HIPCHK(c, hipMemcpy(out, d_out.p, n_out * sizeof(Out), hipMemcpyDeviceToHost));
    return VRT_HIP_OK;
}

extern "C" {

int vrt_hip_transmittance(vrt_hip_ctx *c, const float o[3], const float n[3], const float *s, size_t ns, float *T_out)
{
    if (!c || !o || !n || (ns && (!s || !T_out))) return VRT_HIP_ERR_INVALID;
    return query<float>(c, true, { { s, ns } }, ns, T_out, [&](DevBuf<float> *d, float *T) {
        launch_transmittance(tables(c), o, n, d[0].p, ns, T, c->exp_kind, c->erf_kind, c->stream);
    });
}

int vrt_hip_transmittance_rays(vrt_hip_ctx *c, size_t nrays, const float *origins, const float *dirs, const float *s,
                               float *T_out)
{
    if (!c || (nrays && (!origins || !dirs || !s || !T_out))) return VRT_HIP_ERR_INVALID;
    return query<float>(c, true, { { origins, nrays * 3 }, { dirs, nrays * 3 }, { s, nrays } }, nrays, T_out, [&](DevBuf<float> *d, float *T) {
        launch_transmittance_rays(tables(c), d[0].p, d[1].p, d[2].p, nrays, T, c->exp_kind, c->erf_kind, c->stream);
    });
}

int vrt_hip_transmittance_step(vrt_hip_ctx *c, const float o[3], const float n[3], const float *s, size_t ns, float delta,
                               float *T_out)
{
    if (!c || !o || !n || (ns && (!s || !T_out)) || !(delta > 0.f)) return VRT_HIP_ERR_INVALID;
    // the kernel runs the reference's float loop `t <= s; t += delta`: only arguments for which it ends, and soon (vrt_step_guard.hpp)
    const StepGuard guard = step_guard(s, ns, delta, c->n);
    if (guard.refusal) return fail(c, VRT_HIP_ERR_INVALID, step_refusal_message(guard.refusal));
    return query<float>(c, true, { { s, ns } }, ns, T_out, [&](DevBuf<float> *d, float *T) {
        launch_transmittance_step(tables(c), o, n, d[0].p, ns, delta, T, c->stream);
    });
}

int vrt_hip_density(vrt_hip_ctx *c, size_t npts, const float *pts, float *D_out)
{
    if (!c || (npts && (!pts || !D_out))) return VRT_HIP_ERR_INVALID;
    return query<float>(c, true, { { pts, npts * 3 } }, npts, D_out, [&](DevBuf<float> *d, float *D) {
        launch_density(tables(c), d[0].p, npts, D, c->stream);
    });
}

int vrt_hip_radiance(vrt_hip_ctx *c, size_t nrays, const float *origins, const float *dirs, float *out)
{
    if (!c || (nrays && (!origins || !dirs || !out))) return VRT_HIP_ERR_INVALID;
    return query<float4>(c, true, { { origins, nrays * 3 }, { dirs, nrays * 3 } }, nrays, out, [&](DevBuf<float> *d, float4 *L) {
        launch_radiance(tables(c), d[0].p, d[1].p, nrays, c->iota.p, L, c->exp_kind, c->erf_kind, c->stream);
    });
}

int vrt_hip_eval_erf(vrt_hip_ctx *c, int kind, const float *x, size_t n, float *y)
{
    if (!c || (n && (!x || !y))) return VRT_HIP_ERR_INVALID;
    return query<float>(c, false, { { x, n } }, n, y, [&](DevBuf<float> *d, float *r) { launch_eval_erf(kind, d[0].p, n, r, c->stream); });
}

int vrt_hip_eval_exp(vrt_hip_ctx *c, int kind, const float *x, size_t n, float *y)
{
    if (!c || (n && (!x || !y))) return VRT_HIP_ERR_INVALID;
    return query<float>(c, false, { { x, n } }, n, y, [&](DevBuf<float> *d, float *r) { launch_eval_exp(kind, d[0].p, n, r, c->stream); });
}

} // extern "C"
