"""Ray gradients on the GPU (vrt_hip_radiance_rays_grad_rays*, vrt_hip_transmittance_bundle_grad_rays*): the ray rows of both gradient
bundles against the float64 model of tests/ray_grad_rays_scenes.py, within B = RHO_R * S per component
(tests/test_ray_grad_rays_scenes.py holds model, bound and scenes to account on the CPU); their bits, which are reproducible; what a
call leaves alone; the old entry points; autograd in origins and dirs; and the pose fit."""
import ctypes as C

import numpy as np
import pytest

import ray_grad_rays_scenes as S
from ray_grad_rays_scenes import G, PAIRS, RAY_LCAP, RAY_PL, T, TGRAD_DEPTH, TGRAD_T

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC12345     # a NaN with a payload: any add to it shows, and so does any store
STRIDE = S.RAY_GRAD_STRIDE
WIDE = f"wide {RAY_LCAP + 1} off axis"


def setup(renderer, g, pair="vcl-as", eps=1e-9):
    renderer.set_options(*PAIRS[pair], eps)
    renderer.set_gaussians(g)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def within(got, val, Ssum, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    excess = np.abs(got - val) - S.bound(Ssum)
    j = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[j] <= 0, (what, j, got[j], np.asarray(val)[j], S.bound(Ssum)[j])


def rays_of(sc, rays=None):
    rays = slice(None) if rays is None else rays
    return (sc.o if sc.o.size == 3 else sc.o[rays]), sc.d[rays]


def rad_rows(renderer, sc, rays=None, gr=None, want_table=False):
    """the host form: rows [rays, 6] (and the table's dict)"""
    o, d = rays_of(sc, rays)
    gr = (sc.gr if gr is None else gr)[slice(None) if rays is None else rays]
    table, rows = renderer.radiance_rays_grad(o, d, gr, want_table=want_table, want_rays=True)
    return (S.from_device(rows), table) if want_table else S.from_device(rows)


def device_samples(renderer, case, rays=None):
    rays = slice(None) if rays is None else rays
    if case.wrt == TGRAD_T:
        return case.s[rays] if case.s.ndim == 2 else case.s
    o, d = rays_of(case.sc, rays)
    return renderer.depth_bundle(o, d, case.tau[rays], True)


def trans_rows(renderer, case, s, rays=None, g=None, want_table=False, want_grad_s=False):
    o, d = rays_of(case.sc, rays)
    g = (case.g if g is None else g)[slice(None) if rays is None else rays]
    table, gs, rows = renderer.transmittance_bundle_grad(o, d, s, g, wrt=case.wrt, s_per_ray=s.ndim == 2, want_table=want_table,
                                                         want_grad_s=want_grad_s, want_rays=True)
    return S.from_device(rows), table, gs


def case_of(oracle, mode, name):
    return S.wide_off_axis_case(oracle, mode) if name == WIDE else T.case(oracle, f"{mode} {name}")


# ---- parity with the model ----
RADIANCE = [f"small {n}" for n in (1, 2, 3, 4, 5, 9)] + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64, 128)] + [WIDE]


@pytest.mark.parametrize("eps", S.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("name", RADIANCE)
def test_radiance_rows(renderer, oracle, name, pair, eps):
    sc = S.scene(oracle, name)
    setup(renderer, sc.g, pair, eps)
    renderer.enable_stats(True)
    try:
        rows = rad_rows(renderer, sc)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    val, Ssum = S.model(sc, pair, eps)
    within(rows, val, Ssum, (name, pair, eps))
    lens = [len(l) for l in sc.lists(eps, PAIRS[pair][0])]
    assert st["long_rays"] == sum(n > RAY_PL for n in lens) and st["short_rays"] == sum(n <= RAY_PL for n in lens)
    assert st["scratch_rays"] == sum(n > RAY_LCAP for n in lens)
    assert np.abs(rows).max() > 0


@pytest.mark.parametrize("nrays", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["coherent", "scattered"])
def test_radiance_bundle_sizes(renderer, oracle, kind, nrays):
    sc = S.scene(oracle, f"grid16 {kind}")
    setup(renderer, sc.g)
    val, Ssum = S.model(sc, "vcl-as")
    within(rad_rows(renderer, sc, rays=slice(0, nrays)), val[:nrays], Ssum[:nrays], (kind, nrays))


TRANS = ([f"small 9 ns={ns}" for ns in T.SAMPLE_COUNTS] + [f"{T.CHUNK_SCENE} ns={ns}" for ns in T.CHUNK_COUNTS]
         + [f"small {n}" for n in (1, 2, 3, 5)] + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64)] + [WIDE, "grid16 coherent", "grid16 scattered"])


@pytest.mark.parametrize("pair,eps", [("vcl-as", 1e-9), ("libm-libm", 0.0)])
@pytest.mark.parametrize("mode", ["T", "depth"])
@pytest.mark.parametrize("name", TRANS)
def test_transmittance_and_depth_rows(renderer, oracle, name, mode, pair, eps):
    case = case_of(oracle, mode, name)
    setup(renderer, case.sc.g, pair, eps)
    s = device_samples(renderer, case)
    rows, _, _ = trans_rows(renderer, case, s)
    val, Ssum = S.bundle_trows(case, pair, eps, s=s)
    within(rows, val, Ssum, (case.name, pair, eps))


def test_depths_of_plus_inf_zero_and_nan_give_a_row_of_exact_zeros(renderer, oracle):
    case = T.case(oracle, "depth small 9")
    sc = case.sc
    setup(renderer, sc.g)
    tau = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (len(sc.d), 1))
    depth = renderer.depth_bundle(sc.o, sc.d, tau, True)
    assert np.isinf(depth[:, 0]).all() and (depth[:, 1] == 0).all()
    depth[:, 2] = np.nan
    _, _, rows = renderer.transmittance_bundle_grad(sc.o, sc.d, depth, np.full(depth.shape, 3.0, np.float32), wrt=TGRAD_DEPTH, s_per_ray=True,
                                                    want_table=False, want_grad_s=False, want_rays=True)
    assert (S.from_device(rows) == 0).all()


# ---- the device form ----
def pattern(shape):
    import torch
    return torch.from_numpy(np.full(shape, PATTERN, np.uint32).view(np.float32)).cuda()


def cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in arrays]


def dev_radiance(renderer, t_o, t_d, t_g, nrays=None, table=None, rows=None):
    """the device form over cuda tensors; the results are there after renderer.sync()"""
    nrays = t_d.shape[0] if nrays is None else nrays
    renderer.radiance_rays_grad_rays_device(nrays, t_o.data_ptr(), t_o.numel() != 3, t_d.data_ptr(), t_g.data_ptr(),
                                            d_grad=table.data_ptr() if table is not None else 0, d_grad_rays=rows.data_ptr() if rows is not None else 0)


def dev_trans(renderer, case, t_o, t_d, t_s, t_g, nrays=None, table=None, gs=None, rows=None):
    nrays = t_d.shape[0] if nrays is None else nrays
    renderer.transmittance_bundle_grad_rays_device(nrays, t_o.data_ptr(), t_o.numel() != 3, t_d.data_ptr(), t_s.data_ptr(), t_g.shape[1], t_s.dim() == 2,
                                                   t_g.data_ptr(), case.wrt, d_grad=table.data_ptr() if table is not None else 0,
                                                   d_grad_s=gs.data_ptr() if gs is not None else 0, d_grad_rays=rows.data_ptr() if rows is not None else 0)


def fetch(renderer, t):
    renderer.sync()
    return t.cpu().numpy()


# ---- reproducible bits ----
def test_radiance_rows_are_reproducible(renderer, oracle):
    """two runs, Morton index off / on, table requested or not, host form and device form: the same bits (both kernels run)"""
    import torch
    sc = S.scene(oracle, "grid16 scattered")
    setup(renderer, sc.g)
    assert max(len(l) for l in sc.lists()) > RAY_PL >= min(len(l) for l in sc.lists())
    t_o, t_d, t_g = cuda(sc.o, sc.d, sc.gr)
    nrays = len(sc.d)
    got = []
    try:
        for index in (0, 0, 1):
            renderer.set_ray_index(index)
            _, rows = renderer.radiance_rays_grad(sc.o, sc.d, sc.gr, want_table=False, want_rays=True)
            got.append(np.concatenate([rows["origin"], rows["dir"]], 1))
            table, rows = renderer.radiance_rays_grad(sc.o, sc.d, sc.gr, want_table=True, want_rays=True)
            got.append(np.concatenate([rows["origin"], rows["dir"]], 1))
            assert np.abs(table["mu"]).max() > 0
            for with_table in (False, True):
                buf = pattern((nrays, STRIDE))
                table = torch.zeros((len(sc.g), 12), dtype=torch.float32, device="cuda") if with_table else None
                torch.cuda.synchronize()
                dev_radiance(renderer, t_o, t_d, t_g, table=table, rows=buf)
                out = fetch(renderer, buf)
                got.append(np.concatenate([out[:, 0:3], out[:, 4:7]], 1))
    finally:
        renderer.set_ray_index(0)
    for other in got[1:]:
        np.testing.assert_array_equal(bits(other), bits(got[0]))
    within(got[0], *S.model(sc, "vcl-as"), "scattered")


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_transmittance_rows_are_reproducible(renderer, oracle, mode):
    import torch
    case = T.case(oracle, f"{mode} grid16 scattered")
    sc = case.sc
    setup(renderer, sc.g)
    s = np.ascontiguousarray(device_samples(renderer, case), np.float32)
    t_o, t_d, t_s, t_g = cuda(sc.o, sc.d, s, case.g)
    nrays = len(sc.d)
    got = []
    try:
        for index in (0, 0, 1):
            renderer.set_ray_index(index)
            got.append(trans_rows(renderer, case, s)[0])
            got.append(trans_rows(renderer, case, s, want_table=True, want_grad_s=True)[0])
            for with_table in (False, True):
                buf = pattern((nrays, STRIDE))
                table = torch.zeros((len(sc.g), 12), dtype=torch.float32, device="cuda") if with_table else None
                torch.cuda.synchronize()
                dev_trans(renderer, case, t_o, t_d, t_s, t_g, table=table, rows=buf)
                out = fetch(renderer, buf)
                got.append(np.concatenate([out[:, 0:3], out[:, 4:7]], 1))
    finally:
        renderer.set_ray_index(0)
    for other in got[1:]:
        np.testing.assert_array_equal(bits(other), bits(got[0]))
    assert np.abs(got[0]).max() > 0


# ---- position independence ----
@pytest.mark.parametrize("kernel", ["short", "long"])
def test_a_rays_row_does_not_depend_on_its_place(renderer, oracle, kernel):
    """One ray at index 0, mid-wave, last and alone: the same numbers, for a ray of the lane = ray kernel and one of the one-wave-per-ray
    kernel, radiance and transmittance rows."""
    sc = S.scene(oracle, "grid16 scattered")
    case = T.case(oracle, "T grid16 scattered")
    setup(renderer, sc.g)
    lens = np.array([len(l) for l in sc.lists()])
    r = int(np.nonzero((lens > RAY_PL) if kernel == "long" else ((lens > 4) & (lens <= RAY_PL)))[0][0])
    n = len(sc.d)
    rows, trows = [], []
    for place in (0, 37, n - 1, None):
        if place is None:
            order = np.array([r])
            place = 0
        else:
            order = np.arange(n)
            order[[place, r]] = order[[r, place]]
        rows.append(rad_rows(renderer, sc, rays=order)[place])
        trows.append(trans_rows(renderer, case, case.s[order], rays=order)[0][place])
    for got in (rows, trows):
        assert np.abs(got[0]).max() > 0
        for other in got[1:]:
            assert (other == got[0]).all(), (kernel, other, got[0])


# ---- what is left alone ----
def with_a_ray_that_misses(sc):
    """the bundle (per-ray origins) with one more ray in the middle whose line passes a hundred units from everything"""
    o = np.tile(sc.o, (len(sc.d), 1)) if sc.o.size == 3 else sc.o
    k = len(sc.d) // 2
    o = np.insert(o, k, np.array([100.0, 0.0, -2.0], np.float32), 0)
    d = np.insert(sc.d, k, np.array([0.0, 0.0, 1.0], np.float32), 0)
    assert not G.R.kept(o[k], d[k:k + 1], sc.g, 0.0, 0).any() and not G.R.kept(o[k], d[k:k + 1], sc.g, 0.0, 1).any()
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), k


@pytest.mark.parametrize("kind", ["radiance", "transmittance"])
def test_what_the_ray_output_leaves_alone(renderer, oracle, kind):
    import torch
    sc = S.scene(oracle, "grid16 scattered")
    case = T.case(oracle, "T grid16 scattered")
    setup(renderer, sc.g)
    o, d, k = with_a_ray_that_misses(sc)
    nrays = len(d)
    gr = np.insert(sc.gr, k, 1.0, 0)
    s, g = np.insert(case.s, k, case.s[0], 0), np.insert(case.g, k, 1.0, 0)
    t_o, t_d, t_gr, t_s, t_g = cuda(o, d, gr, s, g)

    def call(table=None, rows=None, nrays=nrays):
        if kind == "radiance":
            dev_radiance(renderer, t_o, t_d, t_gr, nrays=nrays, table=table, rows=rows)
        else:
            dev_trans(renderer, case, t_o, t_d, t_s, t_g, nrays=nrays, table=table, rows=rows)
    # rays only: every row stored, columns 3 and 7 zero, the guard row and a table passed nowhere untouched
    buf, table = pattern((nrays + 1, STRIDE)), pattern((len(sc.g), 12))
    torch.cuda.synchronize()
    call(rows=buf)
    out = fetch(renderer, buf)
    assert (bits(out[:nrays]) != PATTERN).all() and np.isfinite(out[:nrays]).all()
    assert (out[:nrays, 3] == 0).all() and (out[:nrays, 7] == 0).all()
    assert (bits(out[nrays]) == PATTERN).all()
    assert (out[k] == 0).all() and np.abs(out[:nrays]).max() > 0                  # the ray that keeps nothing: exact zeros
    assert (bits(table.cpu().numpy()) == PATTERN).all()
    # fewer rays than the buffer has rows: nothing behind the bundle's last row
    buf2 = pattern((nrays + 1, STRIDE))
    torch.cuda.synchronize()
    call(rows=buf2, nrays=65)
    out2 = fetch(renderer, buf2)
    np.testing.assert_array_equal(bits(out2[:65]), bits(out[:65]))
    assert (bits(out2[65:]) == PATTERN).all()
    # the table only: the ray buffer is not touched
    buf3, zero = pattern((nrays + 1, STRIDE)), torch.zeros((len(sc.g), 12), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    call(table=zero)
    assert (bits(fetch(renderer, buf3)) == PATTERN).all() and np.abs(zero.cpu().numpy()).max() > 0


def test_refusals_and_bundles_of_nothing(renderer, oracle, pkg):
    import torch
    case = T.case(oracle, "T small 5")
    sc = case.sc
    t_o, t_d, t_gr, t_s, t_g = cuda(sc.o, sc.d, sc.gr, case.s, case.g)
    nrays, ns = case.g.shape
    table, gs, buf = pattern((len(sc.g), 12)), pattern((nrays, ns)), pattern((nrays, STRIDE))
    torch.cuda.synchronize()
    L, h = renderer._L, renderer._h
    f32p = C.POINTER(C.c_float)
    host = [np.ascontiguousarray(a, np.float32) for a in (sc.o, sc.d, sc.gr, case.s, case.g)]
    op, dp, grp, sp, gp = (a.ctypes.data_as(f32p) for a in host)
    out, gso, rows = np.full((len(sc.g), 12), -1.0, np.float32), np.full((nrays, ns), -1.0, np.float32), np.full((nrays, STRIDE), -1.0, np.float32)
    outp, gsop, rowsp = (a.ctypes.data_as(f32p) for a in (out, gso, rows))

    def rad_dev(n=nrays, table=table.data_ptr(), rows=buf.data_ptr()):
        return L.vrt_hip_radiance_rays_grad_rays_device(h, n, t_o.data_ptr(), 0, t_d.data_ptr(), t_gr.data_ptr(), table, rows, None)

    def rad_host(n=nrays, table=outp, rows=rowsp):
        return L.vrt_hip_radiance_rays_grad_rays(h, n, op, 0, dp, grp, table, rows)

    def tr_dev(n=nrays, ns=ns, table=table.data_ptr(), gs=gs.data_ptr(), rows=buf.data_ptr()):
        return L.vrt_hip_transmittance_bundle_grad_rays_device(h, n, t_o.data_ptr(), 0, t_d.data_ptr(), t_s.data_ptr(), ns, 1, t_g.data_ptr(), TGRAD_T, table,
                                                               gs, rows, None)

    def tr_host(n=nrays, ns=ns, table=outp, gs=gsop, rows=rowsp):
        return L.vrt_hip_transmittance_bundle_grad_rays(h, n, op, 0, dp, sp, ns, 1, gp, TGRAD_T, table, gs, rows)

    def message(text):
        assert text in L.vrt_hip_last_error(h), (text, L.vrt_hip_last_error(h))
    try:
        setup(renderer, sc.g)
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_SPLINE, 1e-9)                      # a pair with jumps
        for fn, name in ((rad_dev, b"radiance_rays_grad"), (rad_host, b"radiance_rays_grad"), (tr_dev, b"transmittance_bundle_grad"),
                         (tr_host, b"transmittance_bundle_grad")):
            assert fn() == -1
            message(name)
        setup(renderer, sc.g)                                                          # a supported pair again
        assert rad_dev(table=None, rows=None) == -1 and rad_host(table=None, rows=None) == -1          # no output at all
        message(b"NULL grad_radiance or gradient table")
        assert tr_dev(table=None, gs=None, rows=None) == -1 and tr_host(table=None, gs=None, rows=None) == -1
        message(b"neither")
        # nothing to do: no rays, no samples, a scene of no Gaussians
        assert rad_dev(n=0) == 0 and rad_host(n=0) == 0 and tr_dev(n=0) == 0 and tr_host(n=0) == 0
        assert tr_dev(ns=0) == 0 and tr_host(ns=0) == 0
        renderer.set_gaussians(sc.g[:0])
        assert rad_dev() == 0 and rad_host() == 0 and tr_dev() == 0 and tr_host() == 0
        renderer.sync()
        torch.cuda.synchronize()
        for t in (table, gs, buf):
            assert (bits(t.cpu().numpy()) == PATTERN).all()                           # nothing was enqueued
        assert (out == -1.0).all() and (gso == -1.0).all() and (rows == -1.0).all()
    finally:
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)


# ---- the old entry points ----
@pytest.mark.parametrize("name,ray", [("small 9", 0), (f"stack {RAY_PL}|{RAY_PL + 1}", 1)])
def test_the_table_is_the_old_entry_points_table(renderer, oracle, name, ray):
    """A bundle of one ray of the lane = ray kernel: the adds into a row are one lane's, in program order, so the table of the call with
    ray rows is bit for bit the table of the call without; and the row's d origin is minus the sum of the table's d mu within B."""
    import torch
    sc = G.scene(oracle, name)
    case = T.case(oracle, f"T {name}")
    setup(renderer, sc.g)
    assert len(sc.lists()[ray]) <= RAY_PL
    o = sc.origin(ray)
    t_o, t_d, t_gr, t_s, t_g = cuda(o, sc.d[ray:ray + 1], sc.gr[ray:ray + 1], case.samples(ray), case.g[ray:ray + 1])
    tables = [torch.zeros((len(sc.g), 12), dtype=torch.float32, device="cuda") for _ in range(4)]
    bufs = [pattern((1, STRIDE)) for _ in range(2)]
    torch.cuda.synchronize()
    renderer.radiance_rays_grad_device(1, t_o.data_ptr(), 0, t_d.data_ptr(), t_gr.data_ptr(), tables[0].data_ptr())
    dev_radiance(renderer, t_o, t_d, t_gr, table=tables[1], rows=bufs[0])
    renderer.transmittance_bundle_grad_device(1, t_o.data_ptr(), 0, t_d.data_ptr(), t_s.data_ptr(), t_g.shape[1], 0, t_g.data_ptr(), TGRAD_T,
                                              d_grad=tables[2].data_ptr())
    dev_trans(renderer, case, t_o, t_d, t_s, t_g, table=tables[3], rows=bufs[1])
    renderer.sync()
    tables = [t.cpu().numpy() for t in tables]
    np.testing.assert_array_equal(bits(tables[1]), bits(tables[0]))
    np.testing.assert_array_equal(bits(tables[3]), bits(tables[2]))
    rval, rS = S.bundle_rows(sc, "vcl-as", rays=[ray])
    tval, tS = S.bundle_trows(case, "vcl-as", rays=[ray])
    for table, buf, Ssum in ((tables[1], bufs[0], rS[ray]), (tables[3], bufs[1], tS[ray])):
        row = buf.cpu().numpy()[0].astype(np.float64)
        assert np.abs(table[:, 4:7]).max() > 0
        assert (np.abs(row[0:3] + table[:, 4:7].astype(np.float64).sum(0)) <= S.bound(Ssum[0:3])).all()


def test_a_shared_origin_gives_the_rows_of_its_per_ray_copies(renderer, oracle):
    sc = S.scene(oracle, "grid16 coherent")
    case = T.case(oracle, "T grid16 coherent")
    assert sc.o.size == 3
    setup(renderer, sc.g)
    copies = np.tile(sc.o, (len(sc.d), 1))
    _, shared = renderer.radiance_rays_grad(sc.o, sc.d, sc.gr, want_table=False, want_rays=True)
    _, per_ray = renderer.radiance_rays_grad(copies, sc.d, sc.gr, want_table=False, want_rays=True)
    for col in ("origin", "dir"):
        np.testing.assert_array_equal(bits(shared[col]), bits(per_ray[col]))
    np.testing.assert_array_equal(shared["origin"].astype(np.float64).sum(0), per_ray["origin"].astype(np.float64).sum(0))
    a = renderer.transmittance_bundle_grad(sc.o, sc.d, case.s, case.g, want_table=False, want_grad_s=False, want_rays=True)[2]
    b = renderer.transmittance_bundle_grad(copies, sc.d, case.s, case.g, want_table=False, want_grad_s=False, want_rays=True)[2]
    for col in ("origin", "dir"):
        np.testing.assert_array_equal(bits(a[col]), bits(b[col]))
    assert np.abs(a["origin"]).max() > 0


# ---- autograd ----
def parameters(sc, requires_grad):
    import torch
    p = G.params64(sc.g)
    return [torch.tensor(p[k], dtype=torch.float32, device="cuda", requires_grad=requires_grad) for k in ("mu", "albedo", "sigma", "magnitude")]


@pytest.mark.parametrize("shared_origin", [True, False])
@pytest.mark.parametrize("fn", ["radiance_rays", "transmittance_bundle", "depth_bundle"])
def test_autograd_in_origins_and_dirs(renderer, oracle, fn, shared_origin):
    """origins.grad ([3]: the sum over the rays; [nrays, 3]) and the grad of a raw vector behind torch.nn.functional.normalize against
    the model at the directions torch made, within B (a raw vector of length l: B / l); no parameter requires grad: their grads stay None."""
    import torch
    from sgrt_amd import autograd
    mode = {"radiance_rays": None, "transmittance_bundle": "T", "depth_bundle": "depth"}[fn]
    case = T.case(oracle, f"{mode or 'T'} small 9")
    sc = case.sc
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    ps = parameters(sc, False)
    nrays = len(sc.d)
    length = np.linspace(0.5, 2.0, nrays).astype(np.float32)
    raw = torch.tensor(sc.d * length[:, None], device="cuda", requires_grad=True)
    o_host = sc.o if shared_origin else np.tile(sc.o, (nrays, 1))
    origins = torch.tensor(o_host, device="cuda", requires_grad=True)
    dirs = torch.nn.functional.normalize(raw, dim=1)
    used = G.GradScene(sc.name + " torch", sc.g, sc.o, dirs.detach().cpu().numpy(), sc.gr, [])
    assert [list(l) for l in used.lists()] == [list(l) for l in sc.lists()]
    if mode is None:
        out = autograd.radiance_rays(renderer, *ps, origins, dirs)
        (out * torch.from_numpy(sc.gr).cuda()).sum().backward()
        val, Ssum = S.bundle_rows(used, "vcl-as")
    else:
        values = torch.from_numpy(np.ascontiguousarray(case.s if mode == "T" else case.tau, np.float32)).cuda()
        out = (autograd.transmittance_bundle if mode == "T" else autograd.depth_bundle)(renderer, *ps, origins, dirs, values)
        fwd = out.detach().cpu().numpy()
        live = np.isfinite(fwd)
        torch.where(torch.from_numpy(live).cuda(), out * torch.from_numpy(case.g).cuda(), torch.zeros_like(out)).sum().backward()
        probe = T.Case(case.name + " torch", used, case.wrt, case.s if mode == "T" else fwd, np.where(live, case.g, 0.0).astype(np.float32), tau=case.tau)
        val, Ssum = S.bundle_trows(probe, "vcl-as", s=probe.s)
    assert all(p.grad is None for p in ps)
    go, graw = origins.grad.cpu().numpy().astype(np.float64), raw.grad.cpu().numpy().astype(np.float64)
    assert go.shape == o_host.shape and np.abs(go).max() > 0 and np.abs(graw).max() > 0
    if shared_origin:
        within(go, val[:, :3].sum(0), Ssum[:, :3].sum(0), (fn, "origin [3]"))
    else:
        within(go, val[:, :3], Ssum[:, :3], (fn, "origins"))
    # normalize's backward projects onto the tangent plane again (the rows are tangential to rounding) and divides by the length
    within(graw * length[:, None], val[:, 3:], Ssum[:, 3:], (fn, "dirs"))


def test_autograd_with_parameters_and_rays(renderer, oracle):
    """parameters and rays both requiring grad: one call gives the table the old call gives (within its bound) and the ray rows"""
    import torch
    from sgrt_amd import autograd
    sc = G.scene(oracle, "small 9")
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    ps = parameters(sc, True)
    origins = torch.tensor(sc.o, device="cuda", requires_grad=True)
    dirs = torch.tensor(sc.d, device="cuda", requires_grad=True)
    (autograd.radiance_rays(renderer, *ps, origins, dirs) * torch.from_numpy(sc.gr).cuda()).sum().backward()
    val, Ssum = G.model(sc, "vcl-as")
    got = G.table_of({k: p.grad.cpu().numpy() for k, p in zip(("mu", "albedo", "sigma", "magnitude"), ps)})
    assert (np.abs(got - val) <= G.bound(Ssum)).all()
    rval, rS = S.model(sc, "vcl-as")
    within(origins.grad.cpu().numpy(), rval[:, :3].sum(0), rS[:, :3].sum(0), "origin")
    within(dirs.grad.cpu().numpy(), rval[:, 3:], rS[:, 3:], "dirs")


# ---- the pose fit ----
def test_pose_fit_on_the_device(renderer, oracle):
    """The steps of test_ray_grad_rays_scenes.py::test_pose_fit_lowers_the_models_loss through autograd.radiance_rays, the rays built
    with torch ops from the six pose parameters, no parameter of the scene requiring grad: the loss ends at most a fifth of its start
    (half the model's factor of 10, the rest being float32)."""
    import torch
    from sgrt_amd import autograd
    fit = S.PoseFit(oracle)
    renderer.set_options(*PAIRS[fit.PAIR], fit.EPS)
    ps = parameters(fit.sc, False)
    d0 = torch.tensor(fit.d0, dtype=torch.float32, device="cuda")
    o0 = torch.tensor(fit.o0, dtype=torch.float32, device="cuda")
    target = torch.tensor(fit.target, dtype=torch.float32, device="cuda")
    t = torch.tensor(fit.T0, dtype=torch.float32, device="cuda", requires_grad=True)
    w = torch.tensor(fit.W0, dtype=torch.float32, device="cuda", requires_grad=True)

    def loss_of(t, w):
        th = torch.linalg.norm(w)
        zero = torch.zeros((), device="cuda")
        Kx = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
        rot = torch.eye(3, device="cuda") + torch.sin(th) / th * Kx + (1 - torch.cos(th)) / th ** 2 * (Kx @ Kx)
        dirs = torch.nn.functional.normalize(d0 @ rot.T, dim=1)
        return ((autograd.radiance_rays(renderer, *ps, o0 + t, dirs) - target) ** 2).sum()
    losses = []
    for _ in range(fit.STEPS):
        loss = loss_of(t, w)
        losses.append(loss.item())
        gt, gw = torch.autograd.grad(loss, (t, w))
        with torch.no_grad():
            t -= fit.H_T * gt
            w -= fit.H_W * gw
    losses.append(loss_of(t, w).item())
    print("pose fit, device:", losses)
    assert losses[0] > 0 and losses[-1] <= losses[0] / 5, losses
