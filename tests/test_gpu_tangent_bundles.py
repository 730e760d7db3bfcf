"""Tangent bundles on the GPU (vrt_hip_radiance_rays_tangent*, csrc/vrt_ray_tangent_kernel.hip): J . v of the radiance along the
directions of tests/tangent_bundle_scenes.py against its float64 model, within B = RHO_T * S_T per ray and channel; against the merged
gradient kernels through the adjoint identity; against the forward kernel along an albedo direction; and bit for bit where the contract
promises bits.  tests/test_tangent_bundle_scenes.py holds model, bound, scenes and directions to account on the CPU."""
import ctypes as C

import numpy as np
import pytest

import grad_bundle_scenes as G
import ray_bundle_scenes as R
import ray_grad_rays_scenes as RR
import tangent_bundle_scenes as T
from grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC12345     # a NaN with a payload: any store to it shows
SCENES = ([f"small {n}" for n in (1, 2, 3, 4, 5, 9)] + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64, 128)] + [f"wide {RAY_LCAP + 1}"]
          + ["grid16 coherent", "grid16 scattered"])


def test_the_scenes_are_the_gradient_suite(oracle):
    assert [sc.name for sc in G.suite(oracle)] == SCENES


def setup(renderer, g, pair="vcl-as", eps=1e-9):
    renderer.set_options(*PAIRS[pair], eps)
    renderer.set_gaussians(g)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(renderer, sc, v, rv, rays=None):
    """the host form: v [N, 9] or None, rv [nrays, 6] or None -> float32 [rays, 4]"""
    rays = slice(None) if rays is None else rays
    o = sc.o if sc.o.size == 3 else sc.o[rays]
    rows = T.packed_rays(rv, len(sc.d))
    return renderer.radiance_rays_tangent(o, sc.d[rays], T.packed(v, len(sc.g)), None if rows is None else rows[rays])


def dense(sc):
    return T.directions(sc)[0][1:]


_RUNS = {}


def dense_run(renderer, sc):
    """the dense direction of a scene under the default options, run once per session: what the bit tests compare with"""
    if sc.name not in _RUNS:
        setup(renderer, sc.g)
        _RUNS[sc.name] = run(renderer, sc, *dense(sc))
    return _RUNS[sc.name]


# ---- the model: every direction, every scene, both pairs, both cull_eps ----
@pytest.mark.parametrize("eps", T.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("name", SCENES)
def test_model(renderer, oracle, name, pair, eps):
    sc = G.scene(oracle, name)
    setup(renderer, sc.g, pair, eps)
    dirs = T.directions(sc)
    names, v, rv = T.stacked(sc, dirs)
    val, S = T.model(sc, pair, eps, v, rv)
    worst = 0.0
    for q, (dname, vq, rq) in enumerate(dirs):        # every direction on its own, the one-hot ones on the markers among them
        got = run(renderer, sc, vq, rq).astype(np.float64)
        assert np.isfinite(got).all(), (name, dname)
        ratio = np.abs(got - val[q]) / T.bound(S[q])
        worst = max(worst, float(ratio.max()))
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[at] <= 1.0, (name, pair, eps, dname, at, got[at], val[q][at], T.bound(S[q])[at])
    print(f"{name} {pair} eps {eps:g}: worst |got - model| / B = {worst:.3f} over {len(dirs)} directions")


# ---- adjoint: the new kernels against the merged gradient kernels, no model in between ----
@pytest.mark.parametrize("eps", T.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("name", SCENES)
def test_adjoint_of_the_gradient_bundle(renderer, oracle, name, pair, eps):
    """sum_r u_r . (J v)_r by the tangent bundle and <G, v> + <rows, ray v> by radiance_rays_grad of the same renderer, u = the scene's
    gr: they differ by at most sum_r |u_r| RHO_T S_T(r) + sum RHO S |v| + sum RHO_R S_rows |ray v|."""
    sc = G.scene(oracle, name)
    setup(renderer, sc.g, pair, eps)
    u = sc.gr.astype(np.float64)
    table, rows = renderer.radiance_rays_grad(sc.o, sc.d, sc.gr, want_table=True, want_rays=True)
    table, rows = G.table_of(table), RR.from_device(rows)
    _, St = G.model(sc, pair, eps)
    _, Sr = RR.bundle_rows(sc, pair, eps) if name.startswith("wide") else RR.model(sc, pair, eps)
    dirs = [x for x in T.directions(sc) if not x[0].startswith("one-hot")]
    names, v, rv = T.stacked(sc, dirs)
    _, S_T = T.model(sc, pair, eps, v, rv)
    for q, (dname, vq, rq) in enumerate(dirs):
        Jv = run(renderer, sc, vq, rq).astype(np.float64)
        v64, rv64 = v[q].astype(np.float64), rv[q].astype(np.float64)
        lhs = (u * Jv).sum()
        rhs = (table * v64).sum() + (rows * rv64).sum()
        B = (np.abs(u) * T.bound(S_T[q])).sum() + (G.bound(St) * np.abs(v64)).sum() + (RR.bound(Sr) * np.abs(rv64)).sum()
        print(f"{name} {pair} eps {eps:g} {dname}: lhs {lhs:.9e} rhs {rhs:.9e} |diff| / B {abs(lhs - rhs) / B:.3f}")
        assert abs(lhs - rhs) <= B, (name, pair, eps, dname, lhs, rhs, B)


# ---- an albedo direction is a forward bundle of another albedo ----
@pytest.mark.parametrize("eps", T.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("name", SCENES)
def test_albedo_direction_is_the_forward_kernel(renderer, oracle, name, pair, eps):
    """With v = (da, 0, 0, 0) the result is radiance_rays of the scene whose albedo is da (L is linear in the albedo, and the cull
    does not read it), within the forward suite's tolerance for the scene: ray_bundle_scenes.tolerance over TOL and TOL_NOCULL, the
    constants tests/test_gpu_ray_bundles.py imports from there."""
    sc = G.scene(oracle, name)
    da = np.random.default_rng(31).uniform(0.1, 1.0, size=(len(sc.g), 4)).astype(np.float32)
    other = sc.g.copy()
    other["albedo"] = da
    setup(renderer, other, pair, eps)
    want = renderer.radiance_rays(sc.o, sc.d).astype(np.float64)
    setup(renderer, sc.g, pair, eps)
    v = np.zeros((len(sc.g), 9), np.float32)
    v[:, :4] = da
    got = run(renderer, sc, v, None).astype(np.float64)
    lo, hi = R.kept_range(sc.o, sc.d, sc.g, eps, PAIRS[pair][0])
    tol = R.tolerance(lo, hi, float(want.max()), nocull=(eps == 0.0))
    err = np.abs(got - want).max(1)
    print(f"{name} {pair} eps {eps:g}: max err {err.max():.3e}, tolerance {np.min(tol):.1e}..{np.max(tol):.1e}, peak {want.max():.3f}")
    assert np.abs(want).max() > 1e-3
    assert (err <= tol).all(), (name, pair, eps, err.max())


# ---- bits ----
BIT_SCENES = ["grid16 scattered", "grid16 coherent", f"stack {RAY_PL}|{RAY_PL + 1}", f"wide {RAY_LCAP + 1}"]


@pytest.mark.parametrize("name", BIT_SCENES)
def test_bits_index_sort_ordered_and_again(renderer, oracle, name):
    sc = G.scene(oracle, name)
    want = dense_run(renderer, sc)
    assert np.abs(want).max() > 0
    setup(renderer, sc.g)
    v, rv = dense(sc)
    np.testing.assert_array_equal(bits(run(renderer, sc, v, rv)), bits(want), "two runs")
    try:
        for index in (0, 1):
            for sort in (0, 1):
                renderer.set_ray_index(index)
                renderer.set_ray_sort(sort)
                np.testing.assert_array_equal(bits(run(renderer, sc, v, rv)), bits(want), f"index {index} sort {sort}")
        renderer.set_ray_index(0)
        renderer.set_ray_sort(0)
        renderer.set_grad_ordered(1)
        np.testing.assert_array_equal(bits(run(renderer, sc, v, rv)), bits(want), "grad_ordered on")
    finally:
        renderer.set_grad_ordered(0)
        renderer.set_ray_index(0)
        renderer.set_ray_sort(0)


@pytest.mark.parametrize("kind", ["coherent", "scattered"])
def test_bits_bundle_sizes_and_permutation(renderer, oracle, kind):
    sc = G.scene(oracle, f"grid16 {kind}")
    want = dense_run(renderer, sc)
    setup(renderer, sc.g)
    v, rv = dense(sc)
    for n in (1, 63, 64, 65, 130):
        np.testing.assert_array_equal(bits(run(renderer, sc, v, rv, rays=slice(0, n))), bits(want[:n]), f"{n} rays")
    perm = np.random.default_rng(5).permutation(len(sc.d))
    np.testing.assert_array_equal(bits(run(renderer, sc, v, rv, rays=perm)), bits(want[perm]), "a permuted bundle")


def device_call(renderer, sc, table, rows, extra=3, stream=None):
    """the device form over packed arrays (or None); out has `extra` poisoned rows behind the bundle.  Returns out's words."""
    import torch
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (sc.o, sc.d, table, rows)]
    out = torch.from_numpy(np.full((len(sc.d) + extra, 4), PATTERN, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    renderer.radiance_rays_tangent_device(len(sc.d), dev[0].data_ptr(), sc.o.size != 3, dev[1].data_ptr(), 0 if table is None else dev[2].data_ptr(),
                                          0 if rows is None else dev[3].data_ptr(), out.data_ptr())
    renderer.sync()
    return bits(out.cpu().numpy())


@pytest.mark.parametrize("name", ["grid16 scattered", "grid16 coherent", "small 5"])
def test_bits_device_form_and_poison(renderer, oracle, name):
    sc = G.scene(oracle, name)
    want = bits(dense_run(renderer, sc))
    setup(renderer, sc.g)
    v, rv = dense(sc)
    table, rows = T.packed(v, len(sc.g)), T.packed_rays(rv, len(sc.d))
    got = device_call(renderer, sc, table, rows)
    np.testing.assert_array_equal(got[:len(sc.d)], want, "the host form against the device form")
    assert (got[len(sc.d):] == PATTERN).all()                       # nothing behind ray nrays - 1 is written
    # what is never read: columns 9..11, [3] and [7] of the ray rows, the whole rows of Gaussians no ray keeps
    nan = np.float32(np.nan)
    table[:, 9:] = nan
    rows[:, 3] = nan
    rows[:, 7] = nan
    unkept = ~R.kept(sc.o, sc.d, sc.g).any(0)
    if name != "grid16 scattered":
        assert unkept.any()
    if name == "small 5":
        assert unkept[1]                                            # the Gaussian of magnitude 0
    table[unkept] = nan
    got = device_call(renderer, sc, table, rows)
    np.testing.assert_array_equal(got[:len(sc.d)], want, "poison where nothing is read")
    assert (got[len(sc.d):] == PATTERN).all()


# ---- zeros ----
def test_zeros(renderer, oracle):
    base = G.scene(oracle, "small 5")
    # one more ray, far off and parallel to the scene: it keeps nothing
    o = np.concatenate([np.broadcast_to(base.o, base.d.shape), [[0.0, 50.0, 0.0]]]).astype(np.float32)
    d = np.concatenate([base.d, [[1.0, 0.0, 0.0]]]).astype(np.float32)
    sc = G.GradScene("small 5 and a miss", base.g, o, d, None, [])
    for eps in T.EPS:
        assert not R.kept(o, d, sc.g, eps, 1)[-1].any() and R.kept(o, d, sc.g, eps, 1)[:-1].any(1).all()
        setup(renderer, sc.g, "vcl-as", eps)
        v, rv = np.zeros((len(sc.g), 9), np.float32), np.zeros((len(d), 6), np.float32)
        assert (run(renderer, sc, v, None) == 0).all()
        assert (run(renderer, sc, None, rv) == 0).all()
        assert (run(renderer, sc, v, rv) == 0).all()
        rng = np.random.default_rng(3)
        got = run(renderer, sc, rng.uniform(-1, 1, size=v.shape).astype(np.float32), rng.uniform(-1, 1, size=rv.shape).astype(np.float32))
        assert (got[-1] == 0).all() and (got[:-1] != 0).all()       # the ray that keeps nothing: zeros, stored


# ---- refusals ----
def test_refusals(renderer, oracle, pkg):
    import torch
    sc = G.scene(oracle, "small 5")
    v, rv = dense(sc)
    table, rows = T.packed(v, len(sc.g)), T.packed_rays(rv, len(sc.d))
    t_o, t_d, t_t, t_r = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (sc.o, sc.d, table, rows))
    t_out = torch.from_numpy(np.full((len(sc.d), 4), PATTERN, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    dev, host, h, n = renderer._L.vrt_hip_radiance_rays_tangent_device, renderer._L.vrt_hip_radiance_rays_tangent, renderer._h, len(sc.d)
    f32p = C.POINTER(C.c_float)
    o, d = (np.ascontiguousarray(a, np.float32) for a in (sc.o, sc.d))
    out = np.full((n, 4), -1.0, np.float32)
    op, dp, tp, rp, outp = (a.ctypes.data_as(f32p) for a in (o, d, table, rows, out))
    P = [t.data_ptr() for t in (t_o, t_d, t_t, t_r, t_out)]
    try:
        setup(renderer, sc.g)
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_SPLINE, 1e-9)                      # a pair with jumps
        assert dev(h, n, P[0], 0, P[1], P[2], P[3], P[4], None) == -1
        assert b"radiance_rays_tangent" in renderer._L.vrt_hip_last_error(h)
        assert host(h, n, op, 0, dp, tp, rp, outp) == -1
        with pytest.raises(pkg.VrtHipError):
            renderer.radiance_rays_tangent(sc.o, sc.d, table, rows)
        setup(renderer, sc.g)                                                          # a supported pair again
        assert dev(h, n, P[0], 0, P[1], None, None, P[4], None) == -1                 # both inputs NULL
        assert b"neither a tangent table nor ray tangents" in renderer._L.vrt_hip_last_error(h)
        assert dev(h, n, P[0], 0, P[1], P[2], P[3], None, None) == -1                 # NULL out
        assert dev(h, n, None, 0, P[1], P[2], P[3], P[4], None) == -1
        assert dev(h, n, P[0], 0, None, P[2], P[3], P[4], None) == -1
        assert dev(h, 2 ** 32, P[0], 0, P[1], P[2], P[3], P[4], None) == -1
        assert dev(None, n, P[0], 0, P[1], P[2], P[3], P[4], None) == -1
        assert host(h, n, op, 0, dp, None, None, outp) == -1 and host(h, n, op, 0, dp, tp, rp, None) == -1
        assert dev(h, 0, None, 0, None, None, None, None, None) == 0 and host(h, 0, None, 0, None, None, None, None) == 0      # nothing to do
        renderer.set_gaussians(sc.g[:0])                                               # an empty scene
        assert dev(h, n, P[0], 0, P[1], P[2], P[3], P[4], None) == 0 and host(h, n, op, 0, dp, tp, rp, outp) == 0
        renderer.sync()
        torch.cuda.synchronize()
        assert (bits(t_out.cpu().numpy()) == PATTERN).all() and (out == -1.0).all()   # nothing was enqueued, nothing written
    finally:
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        renderer.set_gaussians(sc.g)


# ---- statistics ----
@pytest.mark.parametrize("name", ["grid16 scattered", f"wide {RAY_LCAP + 1}"])
def test_statistics_are_the_radiance_bundles(renderer, oracle, name):
    sc = G.scene(oracle, name)
    setup(renderer, sc.g)
    v, rv = dense(sc)
    renderer.enable_stats(True)
    try:
        for index in (0, 1):
            renderer.set_ray_index(index)
            renderer.radiance_rays(sc.o, sc.d)
            want, want_index = renderer.ray_stats(), renderer.ray_index_stats()
            run(renderer, sc, v, rv)
            assert renderer.ray_stats() == want and want["rays"] == len(sc.d), (name, index)
            assert renderer.ray_index_stats() == want_index and want_index["indexed"] == index, (name, index)
    finally:
        renderer.set_ray_index(0)
        renderer.enable_stats(False)


# ---- torch: forward-mode AD of autograd.radiance_rays ----
def tensors(sc, requires_grad=False):
    import torch
    p = G.params64(sc.g)
    return [torch.tensor(p[k], dtype=torch.float32, device="cuda", requires_grad=requires_grad) for k in ("mu", "albedo", "sigma", "magnitude")]


def split(v):
    """v [N, 9] as the tangents of (mu, albedo, sigma, magnitude)"""
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (v[:, 4:7], v[:, 0:4], v[:, 7], v[:, 8])]


def test_func_jvp_gives_the_direct_calls_bits(renderer, oracle):
    import torch
    from sgrt_amd import autograd
    sc = G.scene(oracle, "small 5")
    want = dense_run(renderer, sc)
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    v, rv = dense(sc)
    t_o, t_d = torch.from_numpy(sc.o).cuda(), torch.from_numpy(sc.d).cuda()
    # one origin for the bundle: its tangent is one row, the same for every ray -- the dense direction's rows differ, so the origin goes per ray
    o_rays = t_o.reshape(1, 3).expand(len(sc.d), 3).contiguous()
    tangents = (*split(v), torch.from_numpy(np.ascontiguousarray(rv[:, :3])).cuda(), torch.from_numpy(np.ascontiguousarray(rv[:, 3:])).cuda())
    L, Jv = torch.func.jvp(lambda *a: autograd.radiance_rays(renderer, *a), (*tensors(sc), o_rays, t_d), tangents)
    np.testing.assert_array_equal(bits(L.cpu().numpy()), bits(renderer.radiance_rays(sc.o, sc.d)))
    np.testing.assert_array_equal(bits(Jv.cpu().numpy()), bits(want))
    # a [3] origin: its tangent moves every ray's origin alike
    shared = next(rq for dname, _, rq in T.directions(sc) if dname == "origin shared")
    _, Jv = torch.func.jvp(lambda o: autograd.radiance_rays(renderer, *tensors(sc), o, t_d), (t_o,), (torch.from_numpy(shared[0, :3].copy()).cuda(),))
    setup(renderer, sc.g)
    np.testing.assert_array_equal(bits(Jv.cpu().numpy()), bits(run(renderer, sc, None, shared)))


def test_forward_ad_passes_only_what_has_a_tangent(renderer, oracle, monkeypatch):
    import torch
    import torch.autograd.forward_ad as fwAD
    from sgrt_amd import autograd
    sc = G.scene(oracle, "small 5")
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    _, rv = dense(sc)
    calls = []
    real = renderer.radiance_rays_tangent_device

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(renderer, "radiance_rays_tangent_device", spy)
    t_o, t_d = torch.from_numpy(sc.o).cuda(), torch.from_numpy(sc.d).cuda()
    with fwAD.dual_level():
        dual = fwAD.make_dual(t_d, torch.from_numpy(np.ascontiguousarray(rv[:, 3:])).cuda())
        Jv = fwAD.unpack_dual(autograd.radiance_rays(renderer, *tensors(sc), t_o, dual)).tangent
        assert len(calls) == 1 and calls[0]["d_tangent"] == 0 and calls[0]["d_ray_tangent"] != 0      # no table
        autograd.radiance_rays(renderer, *tensors(sc), t_o, t_d)
        assert len(calls) == 1                                                                        # no tangent anywhere: nothing issued
    only_dirs = np.zeros_like(rv)
    only_dirs[:, 3:] = rv[:, 3:]
    setup(renderer, sc.g)
    np.testing.assert_array_equal(bits(Jv.cpu().numpy()), bits(run(renderer, sc, None, only_dirs)))


def test_jvp_is_the_adjoint_of_backward(renderer, oracle):
    import torch
    from sgrt_amd import autograd
    sc = G.scene(oracle, "small 5")
    pair, eps = "vcl-as", 1e-9
    renderer.set_options(*PAIRS[pair], eps)
    v, rv = dense(sc)
    u = torch.from_numpy(sc.gr).cuda()
    ps = tensors(sc, requires_grad=True)
    o_rays = torch.from_numpy(np.broadcast_to(sc.o, sc.d.shape).copy()).cuda().requires_grad_(True)
    t_d = torch.from_numpy(sc.d).cuda().requires_grad_(True)
    autograd.radiance_rays(renderer, *ps, o_rays, t_d).mul(u).sum().backward()
    tangents = (*split(v), torch.from_numpy(np.ascontiguousarray(rv[:, :3])).cuda(), torch.from_numpy(np.ascontiguousarray(rv[:, 3:])).cuda())
    rhs = sum(float((p.grad.double() * t.double()).sum()) for p, t in zip((*ps, o_rays, t_d), tangents))
    _, Jv = torch.func.jvp(lambda *a: autograd.radiance_rays(renderer, *a), tuple(t.detach() for t in (*ps, o_rays, t_d)), tangents)
    lhs = float((u.double() * Jv.double()).sum())
    _, v3, rv3 = T.stacked(sc, [("dense", v, rv)])
    _, S_T = T.model(sc, pair, eps, v3, rv3)
    _, St = G.model(sc, pair, eps)
    _, Sr = RR.model(sc, pair, eps)
    B = ((np.abs(sc.gr.astype(np.float64)) * T.bound(S_T[0])).sum() + (G.bound(St) * np.abs(v.astype(np.float64))).sum()
         + (RR.bound(Sr) * np.abs(rv.astype(np.float64))).sum())
    assert abs(lhs - rhs) <= B, (lhs, rhs, B)
