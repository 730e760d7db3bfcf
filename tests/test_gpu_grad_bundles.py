"""Gradient bundles on the GPU (vrt_hip_radiance_rays_grad*, csrc/vrt_ray_grad_kernel.hip) against the float64 model of
tests/grad_bundle_scenes.py, within B = RHO * S per component (tests/test_grad_bundle_scenes.py holds model, bound and scenes to
account on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import grad_bundle_scenes as S
from grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC12345     # a NaN with a payload: any add to it shows, and so does any store


def setup(renderer, g, pair="vcl-as", eps=1e-9):
    renderer.set_options(*PAIRS[pair], eps)
    renderer.set_gaussians(g)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def within(got, val, Ssum, what, mult=1.0):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    excess = np.abs(got - val) - mult * S.bound(Ssum)
    j = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[j] <= 0, (what, j, got[j], val[j], S.bound(Ssum)[j])


def run(renderer, sc, gr=None, rays=None):
    rays = slice(None) if rays is None else rays
    o = sc.o if sc.o.size == 3 else sc.o[rays]
    return S.table_of(renderer.radiance_rays_grad(o, sc.d[rays], (sc.gr if gr is None else gr)[rays]))


# ---- parity with the model: every emitter-chunk residue, RAY_PL either side, the long kernel's rounds, the scratch slot ----
SCENES = [f"small {n}" for n in (1, 2, 3, 4, 5, 9)] + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64, 128)] + [f"wide {RAY_LCAP + 1}"]


@pytest.mark.parametrize("eps", S.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("name", SCENES)
def test_parity(renderer, oracle, name, pair, eps):
    sc = S.scene(oracle, name)
    setup(renderer, sc.g, pair, eps)
    renderer.enable_stats(True)
    try:
        got = run(renderer, sc)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    val, Ssum = S.model(sc, pair, eps)
    within(got, val, Ssum, (name, pair, eps))
    lens = [len(l) for l in sc.lists(eps, PAIRS[pair][0])]
    assert st["rays"] == len(lens) and st["long_rays"] == sum(n > RAY_PL for n in lens) and st["short_rays"] == sum(n <= RAY_PL for n in lens)
    assert st["scratch_rays"] == sum(n > RAY_LCAP for n in lens)
    if name.startswith("stack 32"):
        assert (st["short_rays"], st["long_rays"]) == (1, 1)
    if "small" in name and len(sc.g) >= 5:
        assert (got[1] == 0).all() and np.isfinite(got[2]).all()       # magnitude 0: no ray keeps it, as in the model


# ---- bundle sizes and kinds on the grid scene ----
_PREFIX = {}


def prefix_model(sc, n):
    """The model of the first n rays of the bundle, built up from the pieces between the sizes."""
    sizes = [1, 63, 64, 65, 130]
    if sc.name not in _PREFIX:
        val, Ssum, lo, out = 0.0, 0.0, 0, {}
        for hi in sizes:
            v, s, _ = S.bundle_grad(sc, "vcl-as", 1e-9, rays=range(lo, hi))
            val, Ssum, lo = val + v, Ssum + s, hi
            out[hi] = (val, Ssum)
        _PREFIX[sc.name] = out
    return _PREFIX[sc.name][n]


@pytest.mark.parametrize("nrays", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["coherent", "scattered"])
def test_bundle_sizes(renderer, oracle, kind, nrays):
    sc = S.scene(oracle, f"grid16 {kind}")
    setup(renderer, sc.g)
    val, Ssum = prefix_model(sc, nrays)
    within(run(renderer, sc, rays=slice(0, nrays)), val, Ssum, (kind, nrays))


# ---- what a bundle leaves alone ----
def device_rays(sc):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (sc.o, sc.d, sc.gr)]


def test_untouched_rows_and_columns(renderer, oracle):
    import torch
    sc = S.scene(oracle, "grid16 coherent")
    setup(renderer, sc.g)
    t_o, t_d, t_g = device_rays(sc)
    table = torch.from_numpy(np.full((len(sc.g), 12), PATTERN, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    renderer.radiance_rays_grad_device(len(sc.d), t_o.data_ptr(), 0, t_d.data_ptr(), t_g.data_ptr(), table.data_ptr())
    renderer.sync()
    got = bits(table.cpu().numpy())
    kept = S.R.kept(sc.o, sc.d, sc.g).any(0)
    assert kept.any() and (~kept).any()
    assert (got[~kept] == PATTERN).all()              # a Gaussian that no ray keeps: its row is not written at all
    assert (got[:, 9:] == PATTERN).all()              # columns 9..11 of every row
    # rays with g = 0 change nothing beyond B (every addend is 0: S = 0)
    zero = torch.zeros((len(sc.g), 12), dtype=torch.float32, device="cuda")
    t_z = torch.zeros_like(t_g)
    torch.cuda.synchronize()
    renderer.radiance_rays_grad_device(len(sc.d), t_o.data_ptr(), 0, t_d.data_ptr(), t_z.data_ptr(), zero.data_ptr())
    renderer.sync()
    assert np.abs(zero.cpu().numpy()).max() <= S.bound(np.zeros(1))[0]


def test_device_form_accumulates_and_host_form_overwrites(renderer, oracle):
    import torch
    sc = S.scene(oracle, "grid16 scattered")
    setup(renderer, sc.g)
    val, Ssum = S.model(sc, "vcl-as")
    t_o, t_d, t_g = device_rays(sc)
    table = torch.zeros((len(sc.g), 12), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        st.synchronize()
        for _ in range(2):
            renderer.radiance_rays_grad_device(len(sc.d), t_o.data_ptr(), 1, t_d.data_ptr(), t_g.data_ptr(), table.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
    twice = table.cpu().numpy()
    within(twice[:, :9], 2 * val, 2 * Ssum, "two calls into one table", mult=1.0)      # twice one call, within 2 B
    assert (twice[:, 9:] == 0).all()
    # the host form overwrites what the caller's array held
    f32p = C.POINTER(C.c_float)
    out = np.full((len(sc.g), 12), 1e30, np.float32)
    o, d, g = (np.ascontiguousarray(a, np.float32) for a in (sc.o, sc.d, sc.gr))
    rc = renderer._L.vrt_hip_radiance_rays_grad(renderer._h, len(d), o.ctypes.data_as(f32p), 1, d.ctypes.data_as(f32p), g.ctypes.data_as(f32p),
                                                out.ctypes.data_as(f32p))
    assert rc == 0
    within(out[:, :9], val, Ssum, "host form")
    assert (out[:, 9:] == 0).all()


@pytest.mark.parametrize("name", ["grid16 scattered", f"stack {RAY_PL}|{RAY_PL + 1}", f"wide {RAY_LCAP + 1}"])
def test_morton_index(renderer, oracle, name):
    sc = S.scene(oracle, name)
    setup(renderer, sc.g)
    val, Ssum = S.model(sc, "vcl-as")
    renderer.enable_stats(True)
    try:
        got = {}
        for index in (0, 1):
            renderer.set_ray_index(index)
            renderer.radiance_rays(sc.o, sc.d)
            want, want_index = renderer.ray_stats(), renderer.ray_index_stats()
            got[index] = run(renderer, sc)
            assert renderer.ray_stats() == want and want["rays"] == len(sc.d), (name, index)
            assert renderer.ray_index_stats() == want_index and want_index["indexed"] == index, (name, index)
            within(got[index], val, Ssum, (name, index))
        assert (np.abs(got[1] - got[0]) <= 2 * S.bound(Ssum)).all()
    finally:
        renderer.set_ray_index(0)
        renderer.enable_stats(False)


def test_refusals(renderer, oracle, pkg):
    import torch
    sc = S.scene(oracle, "small 5")
    t_o, t_d, t_g = device_rays(sc)
    table = torch.from_numpy(np.full((len(sc.g), 12), PATTERN, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    dev, host, h, n = renderer._L.vrt_hip_radiance_rays_grad_device, renderer._L.vrt_hip_radiance_rays_grad, renderer._h, len(sc.d)
    f32p = C.POINTER(C.c_float)
    o, d, g = (np.ascontiguousarray(a, np.float32) for a in (sc.o, sc.d, sc.gr))
    out = np.full((len(sc.g), 12), -1.0, np.float32)
    op, dp, gp, outp = (a.ctypes.data_as(f32p) for a in (o, d, g, out))
    try:
        setup(renderer, sc.g)
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_SPLINE, 1e-9)                      # a pair with jumps
        assert dev(h, n, t_o.data_ptr(), 0, t_d.data_ptr(), t_g.data_ptr(), table.data_ptr(), None) == -1
        assert b"radiance_rays_grad" in renderer._L.vrt_hip_last_error(h)
        assert host(h, n, op, 0, dp, gp, outp) == -1
        with pytest.raises(pkg.VrtHipError):
            renderer.radiance_rays_grad(sc.o, sc.d, sc.gr)
        setup(renderer, sc.g)                                                          # a supported pair again
        assert dev(h, n, t_o.data_ptr(), 0, t_d.data_ptr(), None, table.data_ptr(), None) == -1
        assert b"NULL grad_radiance" in renderer._L.vrt_hip_last_error(h)
        assert dev(h, n, t_o.data_ptr(), 0, t_d.data_ptr(), t_g.data_ptr(), None, None) == -1
        assert dev(h, n, None, 0, t_d.data_ptr(), t_g.data_ptr(), table.data_ptr(), None) == -1
        assert dev(h, n, t_o.data_ptr(), 0, None, t_g.data_ptr(), table.data_ptr(), None) == -1
        assert dev(h, 2 ** 32, t_o.data_ptr(), 0, t_d.data_ptr(), t_g.data_ptr(), table.data_ptr(), None) == -1
        assert dev(None, n, t_o.data_ptr(), 0, t_d.data_ptr(), t_g.data_ptr(), table.data_ptr(), None) == -1
        assert host(h, n, op, 0, dp, None, outp) == -1 and host(h, n, op, 0, dp, gp, None) == -1
        assert dev(h, 0, None, 0, None, None, None, None) == 0 and host(h, 0, None, 0, None, None, None) == 0      # nothing to do
        renderer.sync()
        torch.cuda.synchronize()
        assert (bits(table.cpu().numpy()) == PATTERN).all() and (out == -1.0).all()   # nothing was enqueued
    finally:
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)


def test_a_bundle_moves_no_frame_and_no_radiance(renderer, oracle, pkg):
    from sgrt_amd import scene
    g = oracle.grid_scene(16)
    w = h = 64
    cam, _ = scene.cli_camera(w, h)
    setup(renderer, g)
    renderer.set_plane(w, h, *cam.plane())
    renderer.tile_gaussians(2 / 16, 2 / 16, cam.view)
    o, d = S.R.coherent_rays(g, 130)
    gr = S.seeded_gr(len(d), 1)
    img0, rad0 = renderer.render(cam.position)
    L0 = renderer.radiance_rays(o, d)
    grad = renderer.radiance_rays_grad(o, d, gr)
    assert np.abs(grad["mu"]).max() > 0
    L1 = renderer.radiance_rays(o, d)
    img1, rad1 = renderer.render(cam.position)
    np.testing.assert_array_equal(img1, img0)
    np.testing.assert_array_equal(bits(rad1), bits(rad0))
    np.testing.assert_array_equal(bits(L1), bits(L0))
    renderer.clear_tiles()


# ---- autograd ----
def tensors(sc, params=None):
    import torch
    p = S.params64(sc.g) if params is None else params
    return [torch.tensor(p[k], dtype=torch.float32, device="cuda", requires_grad=True) for k in ("mu", "albedo", "sigma", "magnitude")]


def test_autograd_matches_the_binding(renderer, oracle):
    import torch
    from sgrt_amd import autograd
    sc = S.scene(oracle, "small 9")
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    mu, alb, sig, mag = tensors(sc)
    L = autograd.radiance_rays(renderer, mu, alb, sig, mag, torch.from_numpy(sc.o).cuda(), torch.from_numpy(sc.d).cuda())
    L.mul(torch.from_numpy(sc.gr).cuda()).sum().backward()
    got = S.table_of({"albedo": alb.grad.cpu().numpy(), "mu": mu.grad.cpu().numpy(), "sigma": sig.grad.cpu().numpy(), "magnitude": mag.grad.cpu().numpy()})
    want = run(renderer, sc)
    _, Ssum = S.model(sc, "vcl-as")
    assert (np.abs(got - want) <= 2 * S.bound(Ssum)).all()
    np.testing.assert_allclose(L.detach().cpu().numpy(), renderer.radiance_rays(sc.o, sc.d), rtol=0, atol=0)


def descent_case(oracle, pair="vcl-as", eps=1e-9):
    """small 5 with the loss 1/2 |L - L*|^2, L* the radiance of a disturbed scene; the step h (chosen here, on the float64 model) lowers
    the model's loss by at least 0.9 h |grad|^2."""
    sc = S.scene(oracle, "small 5")
    rng = np.random.default_rng(9)
    base = S.params64(sc.g)
    moved = {k: v + 0.05 * rng.normal(size=v.shape) * (v != 0) for k, v in base.items()}
    target = S.forward64(sc, pair, eps, moved)

    def loss(p):
        return 0.5 * ((S.forward64(sc, pair, eps, p) - target) ** 2).sum()
    resid = S.forward64(sc, pair, eps, base) - target
    grad = S.bundle_grad(sc, pair, eps, gr=resid)[0]
    g2 = (grad ** 2).sum()
    h = 1.0
    while True:
        p = {k: base[k] - h * grad[:, S.COLS[k]].reshape(base[k].shape) for k in base}
        if loss(base) - loss(p) >= 0.9 * h * g2:
            return sc, target, h
        h /= 2
        assert h > 1e-6


def test_one_gradient_step_lowers_the_loss(renderer, oracle):
    import torch
    from sgrt_amd import autograd
    sc, target, h = descent_case(oracle)
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    t_o, t_d, t_t = torch.from_numpy(sc.o).cuda(), torch.from_numpy(sc.d).cuda(), torch.tensor(target, dtype=torch.float32, device="cuda")
    ps = tensors(sc)

    def loss_of(ps):
        return 0.5 * ((autograd.radiance_rays(renderer, *ps, t_o, t_d) - t_t) ** 2).sum()
    l0 = loss_of(ps)
    l0.backward()
    g2 = sum(float((p.grad.double() ** 2).sum()) for p in ps)
    assert g2 > 0
    with torch.no_grad():
        stepped = [(p - h * p.grad).detach() for p in ps]
    l1 = loss_of(stepped)
    l0, l1 = l0.item(), l1.item()
    assert l0 - l1 >= 0.5 * h * g2, (l0, l1, h, g2)
