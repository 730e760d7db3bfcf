"""Transmittance gradient bundles on the GPU (vrt_hip_transmittance_bundle_grad*, csrc/vrt_ray_trans_grad_kernel.hip) against the
float64 model of tests/trans_grad_bundle_scenes.py, within B = RHO_T * S per component (tests/test_trans_grad_bundle_scenes.py holds
model, bound and cases to account on the CPU).  In depth mode the samples are the depths the depth bundle returned on the same context,
and the model is evaluated at those."""
import ctypes as C

import numpy as np
import pytest

import grad_bundle_scenes as G
import trans_grad_bundle_scenes as S
from trans_grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL, TGRAD_DEPTH, TGRAD_T

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


def rays_of(case, rays=None):
    sc = case.sc
    rays = slice(None) if rays is None else rays
    return (sc.o if sc.o.size == 3 else sc.o[rays]), sc.d[rays]


def device_samples(renderer, case, rays=None):
    """The samples of the case as the device gets them: its own in T mode, in depth mode what depth_bundle returns for its levels"""
    rays = slice(None) if rays is None else rays
    if case.wrt == TGRAD_T:
        return case.s[rays] if case.s.ndim == 2 else case.s
    o, d = rays_of(case, rays)
    return renderer.depth_bundle(o, d, case.tau[rays], True)


def run(renderer, case, s, rays=None, g=None):
    """(table [N, 5], grad_s [rays, ns]) of the host form"""
    o, d = rays_of(case, rays)
    g = (case.g if g is None else g)[slice(None) if rays is None else rays]
    grad, gs = renderer.transmittance_bundle_grad(o, d, s, g, wrt=case.wrt, s_per_ray=s.ndim == 2)
    return S.table_of(grad), gs


def check(renderer, case, pair, eps, what):
    s = device_samples(renderer, case)
    table, gs = run(renderer, case, s)
    m = S.bundle_tgrad(case, pair, eps, s=s)
    within(table, m.val, m.S, (what, "table"))
    within(gs, m.gs, m.Sgs, (what, "grad_s"))
    return s, table, gs, m


# ---- parity with the model, both modes ----
FULL = [f"small {n}" for n in (1, 2, 3, 5, 9)] + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64)] + [f"wide {RAY_LCAP + 1}"]
ONCE = [n for n in S.PARITY if n not in FULL]       # grid16 coherent (the wave-reduced deposit) and scattered (both kernels), the sample sets


@pytest.mark.parametrize("eps", S.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("mode", ["T", "depth"])
@pytest.mark.parametrize("name", FULL)
def test_parity(renderer, oracle, name, mode, pair, eps):
    case = S.case(oracle, f"{mode} {name}")
    sc = case.sc
    setup(renderer, sc.g, pair, eps)
    s = device_samples(renderer, case)
    renderer.enable_stats(True)
    try:
        table, gs = run(renderer, case, s)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    m = S.bundle_tgrad(case, pair, eps, s=s)
    within(table, m.val, m.S, (case.name, pair, eps, "table"))
    within(gs, m.gs, m.Sgs, (case.name, pair, eps, "grad_s"))
    lens = [len(l) for l in sc.lists(eps, PAIRS[pair][0])]
    assert st["rays"] == len(lens) and st["long_rays"] == sum(n > RAY_PL for n in lens) and st["short_rays"] == sum(n <= RAY_PL for n in lens)
    assert st["scratch_rays"] == sum(n > RAY_LCAP for n in lens)
    if "small" in name and len(sc.g) >= 5:
        assert (table[1] == 0).all() and np.isfinite(table[2]).all()       # magnitude 0: no ray keeps it, as in the model
    if mode == "depth":
        dead = ~(np.isfinite(s) & (s > 0))
        assert (gs[dead] == 0).all()                                       # +inf and 0 depths: per-sample output exactly 0
        assert S.slope_ok(case, pair, s).all()


@pytest.mark.parametrize("mode", ["T", "depth"])
@pytest.mark.parametrize("name", ONCE)
def test_parity_sample_sets_and_grid(renderer, oracle, name, mode):
    case = S.case(oracle, f"{mode} {name}")
    setup(renderer, case.sc.g)
    s, table, gs, m = check(renderer, case, "vcl-as", 1e-9, case.name)
    assert np.abs(table).max() > 0
    if mode == "depth":
        assert (gs[~(np.isfinite(s) & (s > 0))] == 0).all()


def test_depths_of_plus_inf_and_zero_contribute_exactly_nothing(renderer, oracle):
    """A bundle whose depths are all +inf or 0 (levels 0 and 1) leaves a zero table and zero per-sample outputs, whatever g is."""
    case = S.case(oracle, "depth small 9")
    setup(renderer, case.sc.g)
    o, d = rays_of(case)
    tau = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (len(d), 1))
    depth = renderer.depth_bundle(o, d, tau, True)
    assert np.isinf(depth[:, 0]).all() and (depth[:, 1] == 0).all()
    depth[:, 2] = np.nan                                                       # the depth bundle's result for a NaN level
    grad, gs = renderer.transmittance_bundle_grad(o, d, depth, np.full(depth.shape, 3.0, np.float32), wrt=TGRAD_DEPTH, s_per_ray=True)
    assert (S.table_of(grad) == 0).all() and (gs == 0).all()


# ---- bundle sizes and permutations on the grid scene ----
_PREFIX = {}


def prefix_model(case, n):
    """The model of the first n rays of the bundle, built up from the pieces between the sizes."""
    sizes = [1, 63, 64, 65, 130]
    if case.name not in _PREFIX:
        val, Ssum, gs, Sgs, lo, out = 0.0, 0.0, 0.0, 0.0, 0, {}
        for hi in sizes:
            m = S.bundle_tgrad(case, "vcl-as", 1e-9, rays=range(lo, hi))      # the per-sample rows of the other rays stay 0
            val, Ssum, gs, Sgs, lo = val + m.val, Ssum + m.S, gs + m.gs, Sgs + m.Sgs, hi
            out[hi] = (val, Ssum, gs, Sgs)
        _PREFIX[case.name] = out
    return _PREFIX[case.name][n]


@pytest.mark.parametrize("nrays", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["coherent", "scattered"])
def test_bundle_sizes(renderer, oracle, kind, nrays):
    case = S.case(oracle, f"T grid16 {kind}")
    setup(renderer, case.sc.g)
    val, Ssum, mgs, mSgs = prefix_model(case, nrays)
    table, gs = run(renderer, case, case.s[:nrays], rays=slice(0, nrays))
    within(table, val, Ssum, (kind, nrays))
    within(gs, mgs[:nrays], mSgs[:nrays], (kind, nrays, "grad_s"))


def test_a_permuted_bundle_gives_the_same_table_and_the_permuted_grad_s(renderer, oracle):
    case = S.case(oracle, "T grid16 scattered")
    sc = case.sc
    setup(renderer, sc.g)
    m = S.bundle_tgrad(case, "vcl-as", 1e-9)
    perm = np.random.default_rng(5).permutation(len(sc.d))
    grad, gs = renderer.transmittance_bundle_grad(sc.o[perm], sc.d[perm], case.s[perm], case.g[perm], wrt=TGRAD_T, s_per_ray=True)
    within(S.table_of(grad), m.val, m.S, "permuted table")
    within(gs, m.gs[perm], m.Sgs[perm], "permuted grad_s")


# ---- what a bundle leaves alone ----
def device_case(case, s):
    import torch
    sc = case.sc
    s = np.ascontiguousarray(s, np.float32)
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (sc.o, sc.d, s, case.g)]


def pattern(shape):
    import torch
    return torch.from_numpy(np.full(shape, PATTERN, np.uint32).view(np.float32)).cuda()


def test_untouched_rows_and_columns(renderer, oracle):
    import torch
    case = S.case(oracle, "T grid16 coherent")
    sc = case.sc
    g = sc.g.copy()
    kept = G.R.kept(sc.o, sc.d, sc.g).any(0)
    dark = int(np.nonzero(kept)[0][0])
    g["magnitude"][dark] = 0.0                          # a Gaussian of magnitude 0 in the middle of what the rays keep: no ray keeps it
    setup(renderer, g)
    t_o, t_d, t_s, t_g = device_case(case, case.s)
    nrays, ns = case.g.shape
    table, gs = pattern((len(g), 12)), pattern((nrays, ns))
    torch.cuda.synchronize()
    call = renderer.transmittance_bundle_grad_device
    call(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), t_s.data_ptr(), ns, 1, t_g.data_ptr(), TGRAD_T, d_grad=table.data_ptr(), d_grad_s=gs.data_ptr())
    renderer.sync()
    got = bits(table.cpu().numpy())
    kept[dark] = False
    assert kept.any() and (~kept).any()
    assert (got[~kept] == PATTERN).all()                                      # a Gaussian that no ray keeps: its row is not written at all
    assert (got[:, :4] == PATTERN).all() and (got[:, 9:] == PATTERN).all()     # columns 0..3 and 9..11 of every row
    assert (bits(gs.cpu().numpy()) != PATTERN).all()                          # grad_s is stored, every entry
    # grad_s alone leaves no table written, and the reverse
    table, gs2 = pattern((len(g), 12)), pattern((nrays, ns))
    torch.cuda.synchronize()
    call(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), t_s.data_ptr(), ns, 1, t_g.data_ptr(), TGRAD_T, d_grad=0, d_grad_s=gs2.data_ptr())
    renderer.sync()
    assert (bits(table.cpu().numpy()) == PATTERN).all()
    np.testing.assert_array_equal(bits(gs2.cpu().numpy()), bits(gs.cpu().numpy()))
    zero = torch.zeros((len(g), 12), dtype=torch.float32, device="cuda")
    gs3 = pattern((nrays, ns))
    torch.cuda.synchronize()
    call(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), t_s.data_ptr(), ns, 1, t_g.data_ptr(), TGRAD_T, d_grad=zero.data_ptr(), d_grad_s=0)
    renderer.sync()
    assert (bits(gs3.cpu().numpy()) == PATTERN).all() and np.abs(zero.cpu().numpy()).max() > 0


def test_table_forms_and_one_table_for_two_gradients(renderer, oracle):
    import torch
    case = S.case(oracle, "T grid16 scattered")
    sc = case.sc
    setup(renderer, sc.g)
    m = S.bundle_tgrad(case, "vcl-as", 1e-9)
    t_o, t_d, t_s, t_g = device_case(case, case.s)
    nrays, ns = case.g.shape
    table = torch.zeros((len(sc.g), 12), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        st.synchronize()
        for _ in range(2):
            renderer.transmittance_bundle_grad_device(nrays, t_o.data_ptr(), 1, t_d.data_ptr(), t_s.data_ptr(), ns, 1, t_g.data_ptr(), TGRAD_T,
                                                      d_grad=table.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
    twice = table.cpu().numpy()
    within(twice[:, 4:9], 2 * m.val, 2 * m.S, "two calls into one table")       # twice one call, within 2 B
    assert (twice[:, :4] == 0).all() and (twice[:, 9:] == 0).all()
    # the host form overwrites what the caller's arrays held
    f32p = C.POINTER(C.c_float)
    out, gs = np.full((len(sc.g), 12), 1e30, np.float32), np.full((nrays, ns), 1e30, np.float32)
    o, d, s, g = (np.ascontiguousarray(a, np.float32) for a in (sc.o, sc.d, case.s, case.g))
    rc = renderer._L.vrt_hip_transmittance_bundle_grad(renderer._h, nrays, o.ctypes.data_as(f32p), 1, d.ctypes.data_as(f32p), s.ctypes.data_as(f32p), ns, 1,
                                                       g.ctypes.data_as(f32p), TGRAD_T, out.ctypes.data_as(f32p), gs.ctypes.data_as(f32p))
    assert rc == 0
    within(out[:, 4:9], m.val, m.S, "host form")
    within(gs, m.gs, m.Sgs, "host form grad_s")
    assert (out[:, :4] == 0).all() and (out[:, 9:] == 0).all()
    # a radiance gradient and a transmittance gradient into one table: the sum of their models
    rval, rS = G.model(sc, "vcl-as")
    t_gr = torch.from_numpy(sc.gr).cuda()
    table.zero_()
    torch.cuda.synchronize()
    renderer.radiance_rays_grad_device(nrays, t_o.data_ptr(), 1, t_d.data_ptr(), t_gr.data_ptr(), table.data_ptr())
    renderer.transmittance_bundle_grad_device(nrays, t_o.data_ptr(), 1, t_d.data_ptr(), t_s.data_ptr(), ns, 1, t_g.data_ptr(), TGRAD_T, d_grad=table.data_ptr())
    renderer.sync()
    both = table.cpu().numpy().astype(np.float64)
    excess = np.abs(both[:, 4:9] - (rval[:, 4:9] + m.val)) - (G.bound(rS[:, 4:9]) + S.bound(m.S))
    assert excess.max() <= 0
    assert (np.abs(both[:, :4] - rval[:, :4]) <= G.bound(rS[:, :4])).all()


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_a_sample_with_g_zero_is_masked_exactly(renderer, oracle, mode):
    """Samples with g = 0 and s = NaN leave a finite table within B of the bundle without them, and a per-sample output of exactly 0."""
    case = S.case(oracle, f"{mode} grid16 scattered")
    setup(renderer, case.sc.g)
    s = np.array(device_samples(renderer, case), np.float32)
    g = case.g.copy()
    mask = np.random.default_rng(3).random(g.shape) < 0.4
    g[mask] = 0.0
    m = S.bundle_tgrad(case, "vcl-as", 1e-9, s=s, g=g)          # the model of the bundle without them (an addend of weight 0 is no addend)
    s[mask] = np.nan
    table, gs = run(renderer, case, s, g=g)
    within(table, m.val, m.S, (mode, "masked table"))
    within(gs, m.gs, m.Sgs, (mode, "masked grad_s"))
    assert (gs[mask] == 0).all()


@pytest.mark.parametrize("name", ["T grid16 scattered", f"T stack {RAY_PL}|{RAY_PL + 1}", f"depth wide {RAY_LCAP + 1}"])
def test_morton_index(renderer, oracle, name):
    case = S.case(oracle, name)
    sc = case.sc
    setup(renderer, sc.g)
    s = device_samples(renderer, case)
    m = S.bundle_tgrad(case, "vcl-as", 1e-9, s=s)
    renderer.enable_stats(True)
    try:
        got = {}
        for index in (0, 1):
            renderer.set_ray_index(index)
            renderer.radiance_rays(sc.o, sc.d)
            want, want_index = renderer.ray_stats(), renderer.ray_index_stats()
            got[index] = run(renderer, case, s)
            assert renderer.ray_stats() == want and want["rays"] == len(sc.d), (name, index)
            assert renderer.ray_index_stats() == want_index and want_index["indexed"] == index, (name, index)
            within(got[index][0], m.val, m.S, (name, index))
            within(got[index][1], m.gs, m.Sgs, (name, index, "grad_s"))
        assert (np.abs(got[1][0] - got[0][0]) <= 2 * S.bound(m.S)).all()
    finally:
        renderer.set_ray_index(0)
        renderer.enable_stats(False)


def test_refusals(renderer, oracle, pkg):
    import torch
    case = S.case(oracle, "T small 5")
    sc = case.sc
    t_o, t_d, t_s, t_g = device_case(case, case.s)
    nrays, ns = case.g.shape
    table, gs = pattern((len(sc.g), 12)), pattern((nrays, ns))
    torch.cuda.synchronize()
    L, h = renderer._L, renderer._h
    f32p = C.POINTER(C.c_float)
    o, d, s, g = (np.ascontiguousarray(a, np.float32) for a in (sc.o, sc.d, case.s, case.g))
    out, gso = np.full((len(sc.g), 12), -1.0, np.float32), np.full((nrays, ns), -1.0, np.float32)
    op, dp, sp, gp, outp, gsop = (a.ctypes.data_as(f32p) for a in (o, d, s, g, out, gso))
    P = dict(o=t_o.data_ptr(), d=t_d.data_ptr(), s=t_s.data_ptr(), g=t_g.data_ptr(), table=table.data_ptr(), gs=gs.data_ptr(), n=nrays, ns=ns, wrt=TGRAD_T, ctx=h)

    def dev(**kw):
        a = {**P, **kw}
        return L.vrt_hip_transmittance_bundle_grad_device(a["ctx"], a["n"], a["o"], 0, a["d"], a["s"], a["ns"], 1, a["g"], a["wrt"], a["table"], a["gs"], None)

    def host(**kw):
        a = {**dict(o=op, d=dp, s=sp, g=gp, table=outp, gs=gsop, n=nrays, ns=ns, wrt=TGRAD_T), **kw}
        return L.vrt_hip_transmittance_bundle_grad(h, a["n"], a["o"], 0, a["d"], a["s"], a["ns"], 1, a["g"], a["wrt"], a["table"], a["gs"])

    def message(text):
        assert text in L.vrt_hip_last_error(h), (text, L.vrt_hip_last_error(h))
    try:
        setup(renderer, sc.g)
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_SPLINE, 1e-9)                      # a pair with jumps
        assert dev() == -1
        message(b"transmittance_bundle_grad")
        assert host() == -1
        with pytest.raises(pkg.VrtHipError):
            renderer.transmittance_bundle_grad(sc.o, sc.d, case.s, case.g)
        setup(renderer, sc.g)                                                          # a supported pair again
        for null in ("o", "d", "s", "g"):
            assert dev(**{null: None}) == -1 and host(**{null: None}) == -1, null
            message(b"NULL")
        assert dev(table=None, gs=None) == -1 and host(table=None, gs=None) == -1      # both outputs NULL
        message(b"neither")
        for wrt in (-1, 2):
            assert dev(wrt=wrt) == -1 and host(wrt=wrt) == -1
            message(b"wrt")
        assert dev(n=2 ** 32) == -1
        message(b"2^32")
        assert dev(ns=2 ** 62) == -1
        message(b"does not fit")
        assert dev(ctx=None) == -1
        # nothing to do: no rays, no samples, NULLs allowed
        assert dev(n=0, o=None, d=None, s=None, g=None, table=None, gs=None) == 0 and host(n=0, o=None, d=None, s=None, g=None, table=None, gs=None) == 0
        assert dev(ns=0, s=None, g=None) == 0 and host(ns=0, s=None, g=None) == 0
        renderer.set_gaussians(sc.g[:0])                                               # a scene of no Gaussians
        assert dev() == 0 and host() == 0
        renderer.sync()
        torch.cuda.synchronize()
        assert (bits(table.cpu().numpy()) == PATTERN).all() and (bits(gs.cpu().numpy()) == PATTERN).all()      # nothing was enqueued
        assert (out == -1.0).all() and (gso == -1.0).all()
    finally:
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)


def test_a_bundle_moves_no_frame_no_radiance_and_no_T(renderer, oracle, pkg):
    from sgrt_amd import scene
    g = oracle.grid_scene(16)
    w = h = 64
    cam, _ = scene.cli_camera(w, h)
    setup(renderer, g)
    renderer.set_plane(w, h, *cam.plane())
    renderer.tile_gaussians(2 / 16, 2 / 16, cam.view)
    o, d = G.R.coherent_rays(g, 130)
    s = np.linspace(0.0, 8.0, 5).astype(np.float32)
    gT = S.seeded_g(len(d), len(s), 1)
    img0, rad0 = renderer.render(cam.position)
    L0, T0 = renderer.radiance_rays(o, d), renderer.transmittance_bundle(o, d, s)
    depth0 = renderer.depth_bundle(o, d, np.array([0.5], np.float32))
    grad, gs = renderer.transmittance_bundle_grad(o, d, s, gT)
    assert np.abs(grad["mu"]).max() > 0
    renderer.transmittance_bundle_grad(o, d, depth0, S.seeded_g(len(d), 1, 2), wrt=TGRAD_DEPTH, s_per_ray=True)
    L1, T1 = renderer.radiance_rays(o, d), renderer.transmittance_bundle(o, d, s)
    img1, rad1 = renderer.render(cam.position)
    np.testing.assert_array_equal(img1, img0)
    np.testing.assert_array_equal(bits(rad1), bits(rad0))
    np.testing.assert_array_equal(bits(L1), bits(L0))
    np.testing.assert_array_equal(bits(T1), bits(T0))
    renderer.clear_tiles()


# ---- autograd ----
def tensors(sc, params=None):
    import torch
    p = G.params64(sc.g) if params is None else params
    return [torch.tensor(p[k], dtype=torch.float32, device="cuda", requires_grad=True) for k in ("mu", "albedo", "sigma", "magnitude")]


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_autograd_matches_the_binding(renderer, oracle, mode):
    import torch
    from sgrt_amd import autograd
    case = S.case(oracle, f"{mode} small 9")
    sc = case.sc
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    mu, alb, sig, mag = tensors(sc)
    t_o, t_d, t_g = torch.from_numpy(sc.o).cuda(), torch.from_numpy(sc.d).cuda(), torch.from_numpy(case.g).cuda()
    v = torch.tensor(case.s if mode == "T" else case.tau, dtype=torch.float32, device="cuda", requires_grad=True)
    fn = autograd.transmittance_bundle if mode == "T" else autograd.depth_bundle
    out = fn(renderer, mu, alb, sig, mag, t_o, t_d, v)
    fwd = out.detach().cpu().numpy()
    live = np.isfinite(fwd)
    torch.where(torch.from_numpy(live).cuda(), out * t_g, torch.zeros_like(out)).sum().backward()
    assert alb.grad is None
    got = S.table_of({"mu": mu.grad.cpu().numpy(), "sigma": sig.grad.cpu().numpy(), "magnitude": mag.grad.cpu().numpy()})
    if mode == "T":
        np.testing.assert_array_equal(bits(fwd), bits(renderer.transmittance_bundle(sc.o, sc.d, case.s)))
        s = case.s
    else:
        np.testing.assert_array_equal(bits(fwd), bits(renderer.depth_bundle(sc.o, sc.d, case.tau, True)))
        s = fwd
    g = np.where(live, case.g, 0.0).astype(np.float32)
    table, gs = run(renderer, case, s, g=g)
    m = S.bundle_tgrad(case, "vcl-as", 1e-9, s=s, g=g)
    assert (np.abs(got - table) <= 2 * S.bound(m.S)).all()
    want_v = gs if v.dim() == 2 else gs.sum(0)
    assert (np.abs(v.grad.cpu().numpy() - want_v) <= 2 * S.bound(m.Sgs if v.dim() == 2 else m.Sgs.sum(0))).all()


def descent_case(oracle, mode, pair="vcl-as", eps=1e-9):
    """small 5 with a loss on T (a mask loss, sum (T - T*)^2, T* the transmittance of a disturbed scene) or on the median depth (sum over
    the rays that reach tau = 0.5 of (depth - depth*)^2, depth* 0.1 in front); the step h (chosen here, on the float64 model, as
    test_gpu_grad_bundles.descent_case does) lowers the model's loss by at least 0.9 h |grad|^2."""
    case = S.case(oracle, f"{mode} small 5")
    sc = case.sc
    base = S.params64(sc.g)
    lists = sc.lists(eps, PAIRS[pair][0])
    nrays = len(sc.d)
    if mode == "T":
        rng = np.random.default_rng(9)
        moved = {k: v + 0.05 * rng.normal(size=v.shape) * (v != 0) for k, v in base.items()}
        values = case.s
        target = S.bundle_tgrad(case, pair, eps, params=moved).T

        def forward(p):
            return S.bundle_tgrad(case, pair, eps, params=p).T
        live = np.ones(target.shape, bool)
    else:
        values = np.full((nrays, 1), 0.5, np.float32)

        def forward(p):
            return np.stack([S.root(sc, pair, r, lists[r], values[r], g=p, tol=1e-12) for r in range(nrays)])
        d0 = forward(base)
        live = np.isfinite(d0) & (d0 > 0)
        assert live.any()
        target = np.where(live, d0 - 0.1, 0.0)

    def loss(p):
        return (np.where(live, forward(p) - target, 0.0) ** 2).sum()
    f0 = forward(base)
    resid = np.where(live, 2 * (f0 - target), 0.0)
    probe = S.Case(case.name + " descent", sc, case.wrt, values if mode == "T" else None, resid.astype(np.float64))
    grad = S.bundle_tgrad(probe, pair, eps, s=values if mode == "T" else np.where(live, f0, np.inf)).val
    g2 = (grad ** 2).sum()
    cols = {"mu": slice(0, 3), "sigma": 3, "magnitude": 4}
    h = 1.0
    while True:
        p = {k: base[k] - h * grad[:, cols[k]].reshape(base[k].shape) for k in base}
        if loss(base) - loss(p) >= 0.9 * h * g2:
            return sc, values, target, live, h
        h /= 2
        assert h > 1e-6


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_one_gradient_step_lowers_the_loss(renderer, oracle, mode):
    import torch
    from sgrt_amd import autograd
    sc, values, target, live, h = descent_case(oracle, mode)
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    t_o, t_d = torch.from_numpy(sc.o).cuda(), torch.from_numpy(sc.d).cuda()
    t_v, t_t = torch.from_numpy(np.ascontiguousarray(values, np.float32)).cuda(), torch.tensor(target, dtype=torch.float32, device="cuda")
    t_live = torch.from_numpy(live).cuda()
    fn = autograd.transmittance_bundle if mode == "T" else autograd.depth_bundle
    ps = tensors(sc)

    def loss_of(ps):
        out = fn(renderer, *ps, t_o, t_d, t_v)
        return (torch.where(t_live, out - t_t, torch.zeros_like(out)) ** 2).sum()
    l0 = loss_of(ps)
    l0.backward()
    g2 = sum(float((p.grad.double() ** 2).sum()) for p in ps if p.grad is not None)
    assert g2 > 0
    with torch.no_grad():
        stepped = [(p - h * p.grad).detach() if p.grad is not None else p.detach() for p in ps]
    l1 = loss_of(stepped)
    l0, l1 = l0.item(), l1.item()
    assert l0 - l1 >= 0.5 * h * g2, (mode, l0, l1, h, g2)
