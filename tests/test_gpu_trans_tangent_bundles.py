"""Transmittance tangent bundles on the GPU (vrt_hip_transmittance_bundle_tangent*, csrc/vrt_ray_trans_tangent_kernel.hip): J . v of the
transmittance and of the depth along the directions of tests/trans_tangent_bundle_scenes.py against its float64 model, within
B = RHO_TT * S_T per ray and sample; against the merged transmittance gradient kernels through the adjoint identity; and bit for bit where
the contract promises bits.  The cases are exactly the transmittance gradient suite's (tests/trans_grad_bundle_scenes.py); in depth mode
the samples are the depths the depth bundle returned on the same context.  tests/test_trans_tangent_bundle_scenes.py holds model, bound,
cases and directions to account on the CPU."""
import ctypes as C

import numpy as np
import pytest

import grad_bundle_scenes as G
import ray_bundle_scenes as R
import ray_grad_rays_scenes as RR
import trans_grad_bundle_scenes as T
import trans_tangent_bundle_scenes as TT
from trans_grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL, TGRAD_DEPTH, TGRAD_T

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC12345     # a NaN with a payload: any store to it shows
# small lists; the residues of RAY_SG; the short / long border and a second round of lanes.  The long kernel stages no samples: no chunk cases.
FULL = ([f"small {n}" for n in (1, 2, 3, 5, 9)] + [f"small 9 ns={ns}" for ns in T.SAMPLE_COUNTS] + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64)])
ONCE = [f"wide {RAY_LCAP + 1}", "grid16 coherent", "grid16 scattered"]      # the scratch slot; both kernels in one bundle, and RHO_TT's worst case


def test_the_cases_are_the_transmittance_gradient_suites(oracle):
    assert set(FULL + ONCE) <= set(T.PARITY) and T.SG == 4 and sorted(ns % T.SG for ns in T.SAMPLE_COUNTS) == [0, 1, 1, 1, 3]


def setup(renderer, g, pair="vcl-as", eps=1e-9):
    renderer.set_options(*PAIRS[pair], eps)
    renderer.set_gaussians(g)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rays_of(case, rays=None):
    sc = case.sc
    rays = slice(None) if rays is None else rays
    return (sc.o if sc.o.size == 3 else sc.o[rays]), sc.d[rays]


def device_samples(renderer, case):
    """The samples of the case as the device gets them: its own in T mode, in depth mode what depth_bundle returns for its levels"""
    if case.wrt == TGRAD_T:
        return case.s
    o, d = rays_of(case)
    return renderer.depth_bundle(o, d, case.tau, True)


def run(renderer, case, s, v, rv, sd, rays=None):
    """the host form: v [N, 5] or None, rv [nrays, 6] or None, sd [nrays, ns] / [ns] or None -> float32 [rays, ns]"""
    sel = slice(None) if rays is None else rays
    o, d = rays_of(case, sel)
    rows = TT.packed_rays(rv, len(case.sc.d))
    return renderer.transmittance_bundle_tangent(o, d, s[sel] if s.ndim == 2 else s, tangent=TT.packed(v, len(case.sc.g)),
                                                 ray_tangent=None if rows is None else rows[sel],
                                                 s_tangent=None if sd is None else (sd[sel] if sd.ndim == 2 else sd), wrt=case.wrt, s_per_ray=s.ndim == 2)


def dense(case):
    return TT.directions(case)[0][1:]


_RUNS = {}


def dense_run(renderer, case):
    """(samples, the dense direction's result) of a case under the default options, run once per session: what the bit tests compare with"""
    if case.name not in _RUNS:
        setup(renderer, case.sc.g)
        s = device_samples(renderer, case)
        _RUNS[case.name] = (s, run(renderer, case, s, *dense(case)))
    return _RUNS[case.name]


def check_model(renderer, case, pair, eps):
    setup(renderer, case.sc.g, pair, eps)
    s = device_samples(renderer, case)
    dirs = TT.directions(case)
    names, v, rv, sd = TT.stacked(case, dirs)
    val, S = TT.model(case, pair, eps, s, v, rv, sd)
    dead = np.zeros(case.g.shape, bool)
    if case.wrt == TGRAD_DEPTH:
        dead = ~(np.isfinite(s) & (s > 0))
        assert T.slope_ok(case, pair, s).all() and not dead.all()
    worst = 0.0
    for q, (dname, vq, rq, sq) in enumerate(dirs):        # every direction on its own, the one-hot ones on the markers among them
        got = run(renderer, case, s, vq, rq, sq).astype(np.float64)
        assert np.isfinite(got).all(), (case.name, dname)
        assert (got[dead] == 0).all(), (case.name, dname)                     # +inf and 0 depths: exactly 0
        ratio = np.abs(got - val[q]) / TT.bound(S[q])
        worst = max(worst, float(ratio.max()))
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[at] <= 1.0, (case.name, pair, eps, dname, at, got[at], val[q][at], TT.bound(S[q])[at])
    print(f"{case.name} {pair} eps {eps:g}: worst |got - model| / B = {worst:.3f} over {len(dirs)} directions")


# ---- the model: every direction, both modes, both pairs, both cull_eps ----
@pytest.mark.parametrize("eps", T.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("mode", ["T", "depth"])
@pytest.mark.parametrize("name", FULL)
def test_model(renderer, oracle, name, mode, pair, eps):
    case = T.case(oracle, f"{mode} {name}")
    check_model(renderer, case, pair, eps)
    if name == f"stack {RAY_PL}|{RAY_PL + 1}":
        assert [len(l) for l in case.sc.lists(eps, PAIRS[pair][0])] == [RAY_PL + 1, RAY_PL]       # one ray to each kernel


@pytest.mark.parametrize("mode", ["T", "depth"])
@pytest.mark.parametrize("name", ONCE)
def test_model_wide_and_grid(renderer, oracle, name, mode):
    check_model(renderer, T.case(oracle, f"{mode} {name}"), "vcl-as", 1e-9)


# ---- adjoint: the new kernels against the merged gradient kernels, no model in between ----
@pytest.mark.parametrize("pair,eps", [("vcl-as", 1e-9), ("libm-libm", 0.0)])
@pytest.mark.parametrize("mode", ["T", "depth"])
@pytest.mark.parametrize("name", FULL + ONCE)
def test_adjoint_of_the_gradient_bundle(renderer, oracle, name, mode, pair, eps):
    """sum_rk g_rk (J v)_rk by the tangent bundle and <table, v> + <ray rows, ray v> + <grad_s, sample v> by transmittance_bundle_grad of
    the same renderer, g = the case's: they differ by at most the sum of the three bounds of the reverse side,
    sum RHO_T S |v| + sum RHO_R S_rows |ray v| + sum RHO_T S_gs |sample v|."""
    case = T.case(oracle, f"{mode} {name}")
    sc = case.sc
    setup(renderer, sc.g, pair, eps)
    s = device_samples(renderer, case)
    o, d = rays_of(case)
    u = case.g.astype(np.float64)
    table, gs, rows = renderer.transmittance_bundle_grad(o, d, s, case.g, wrt=case.wrt, s_per_ray=s.ndim == 2, want_rays=True)
    table, rows, gs = T.table_of(table), RR.from_device(rows), gs.astype(np.float64)
    m = T.bundle_tgrad(case, pair, eps, s=s)
    _, Sr = RR.bundle_trows(case, pair, eps, s=s)
    dirs = [x for x in TT.directions(case) if not x[0].startswith("one-hot")]
    names, v, rv, sd = TT.stacked(case, dirs)
    for q, (dname, vq, rq, sq) in enumerate(dirs):
        Jv = run(renderer, case, s, vq, rq, sq).astype(np.float64)
        v64, rv64, sd64 = v[q].astype(np.float64), rv[q].astype(np.float64), sd[q].astype(np.float64)
        lhs = (u * Jv).sum()
        rhs = (table * v64).sum() + (rows * rv64).sum() + (gs * sd64).sum()
        B = (T.bound(m.S) * np.abs(v64)).sum() + (RR.bound(Sr) * np.abs(rv64)).sum() + (T.bound(m.Sgs) * np.abs(sd64)).sum()
        print(f"{case.name} {pair} eps {eps:g} {dname}: lhs {lhs:.9e} rhs {rhs:.9e} |diff| / B {abs(lhs - rhs) / B:.3f}")
        assert abs(lhs - rhs) <= B, (case.name, pair, eps, dname, lhs, rhs, B)


@pytest.mark.parametrize("name", ["small 9", f"stack {RAY_PL}|{RAY_PL + 1}", "grid16 scattered"])
def test_a_sample_direction_is_grad_s_of_ones(renderer, oracle, name):
    """T mode, samples only: out[r, k] = T_k S_k ds_k, and T_k S_k is the reverse call's grad_s with g = 1."""
    case = T.case(oracle, f"T {name}")
    setup(renderer, case.sc.g)
    o, d = rays_of(case)
    ones = np.ones(case.g.shape, np.float32)
    _, TS = renderer.transmittance_bundle_grad(o, d, case.s, ones, wrt=TGRAD_T, s_per_ray=case.s.ndim == 2, want_table=False)
    sd = next(x[3] for x in TT.directions(case) if x[0] == "samples")
    got = run(renderer, case, case.s, None, None, sd).astype(np.float64)
    m = T.bundle_tgrad(case, "vcl-as", 1e-9, g=ones)
    want = TS.astype(np.float64) * sd
    assert np.abs(want).max() > 0
    assert (np.abs(got - want) <= (TT.bound(m.Sgs) + T.bound(m.Sgs)) * np.abs(sd)).all()


def test_depths_of_plus_inf_zero_and_nan_give_exact_zeros(renderer, oracle):
    case = T.case(oracle, "depth small 9")
    setup(renderer, case.sc.g)
    o, d = rays_of(case)
    tau = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (len(d), 1))
    depth = renderer.depth_bundle(o, d, tau, True)
    assert np.isinf(depth[:, 0]).all() and (depth[:, 1] == 0).all()
    depth[:, 2] = np.nan                                                       # the depth bundle's result for a NaN level
    rng = np.random.default_rng(11)
    v, rv, sd = (rng.uniform(-1, 1, size=sh).astype(np.float32) for sh in ((len(case.sc.g), 5), (len(d), 6), depth.shape))
    got = renderer.transmittance_bundle_tangent(o, d, depth, TT.packed(v, len(case.sc.g)), TT.packed_rays(rv, len(d)), sd, wrt=TGRAD_DEPTH, s_per_ray=True)
    assert (bits(got) == 0).all()


# ---- bits ----
BIT_CASES = ["T grid16 scattered", "depth grid16 coherent", f"T stack {RAY_PL}|{RAY_PL + 1}", "depth stack 64|65", f"depth wide {RAY_LCAP + 1}"]


@pytest.mark.parametrize("name", BIT_CASES)
def test_bits_index_sort_ordered_and_again(renderer, oracle, name):
    case = T.case(oracle, name)
    s, want = dense_run(renderer, case)
    assert np.abs(want).max() > 0
    setup(renderer, case.sc.g)
    v, rv, sd = dense(case)
    np.testing.assert_array_equal(bits(run(renderer, case, s, v, rv, sd)), bits(want), "two runs")
    try:
        for index in (0, 1):
            for sort in (0, 1):
                renderer.set_ray_index(index)
                renderer.set_ray_sort(sort)
                np.testing.assert_array_equal(bits(run(renderer, case, s, v, rv, sd)), bits(want), f"index {index} sort {sort}")
        renderer.set_ray_index(0)
        renderer.set_ray_sort(0)
        renderer.set_grad_ordered(1)
        np.testing.assert_array_equal(bits(run(renderer, case, s, v, rv, sd)), bits(want), "grad_ordered on")
    finally:
        renderer.set_grad_ordered(0)
        renderer.set_ray_index(0)
        renderer.set_ray_sort(0)


@pytest.mark.parametrize("name", ["T grid16 coherent", "T grid16 scattered", "depth grid16 scattered"])
def test_bits_bundle_sizes_and_permutation(renderer, oracle, name):
    case = T.case(oracle, name)
    s, want = dense_run(renderer, case)
    assert s.ndim == 2
    setup(renderer, case.sc.g)
    v, rv, sd = dense(case)
    for n in (1, 63, 64, 65, 130):
        np.testing.assert_array_equal(bits(run(renderer, case, s, v, rv, sd, rays=slice(0, n))), bits(want[:n]), f"{n} rays")
    perm = np.random.default_rng(5).permutation(len(case.sc.d))
    np.testing.assert_array_equal(bits(run(renderer, case, s, v, rv, sd, rays=perm)), bits(want[perm]), "a permuted bundle")


@pytest.mark.parametrize("name", ["T small 9", f"T stack {RAY_PL}|{RAY_PL + 1}", "depth grid16 scattered"])
def test_bits_shared_and_per_ray_sample_tangents(renderer, oracle, name):
    case = T.case(oracle, name)
    setup(renderer, case.sc.g)
    s = device_samples(renderer, case)
    v, rv, _ = dense(case)
    shared = next(x[3] for x in TT.directions(case) if x[0] == "samples shared")
    per_ray = np.ascontiguousarray(np.broadcast_to(shared, case.g.shape))
    a, b = run(renderer, case, s, v, rv, shared), run(renderer, case, s, v, rv, per_ray)
    assert np.abs(a).max() > 0
    np.testing.assert_array_equal(bits(a), bits(b))


def device_call(renderer, case, s, table, rows, sd, extra=3):
    """the device form over packed arrays (or None); out has `extra` poisoned rows behind the bundle.  Returns out's words."""
    import torch
    sc = case.sc
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (sc.o, sc.d, s, table, rows, sd)]
    nrays, ns = case.g.shape
    out = torch.from_numpy(np.full((nrays + extra, ns), PATTERN, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    renderer.transmittance_bundle_tangent_device(nrays, dev[0].data_ptr(), sc.o.size != 3, dev[1].data_ptr(), dev[2].data_ptr(), ns, s.ndim == 2, case.wrt,
                                                 d_tangent=0 if table is None else dev[3].data_ptr(), d_ray_tangent=0 if rows is None else dev[4].data_ptr(),
                                                 d_s_tangent=0 if sd is None else dev[5].data_ptr(), s_tangent_per_ray=sd is None or sd.ndim == 2,
                                                 d_out=out.data_ptr())
    renderer.sync()
    return bits(out.cpu().numpy())


@pytest.mark.parametrize("name", ["T grid16 scattered", "depth grid16 coherent", "T small 5"])
def test_bits_device_form_and_poison(renderer, oracle, name):
    case = T.case(oracle, name)
    sc = case.sc
    s, want = dense_run(renderer, case)
    want = bits(want)
    setup(renderer, sc.g)
    v, rv, sd = dense(case)
    nrays = len(sc.d)
    table, rows = TT.packed(v, len(sc.g)), TT.packed_rays(rv, nrays)
    got = device_call(renderer, case, s, table, rows, sd)
    np.testing.assert_array_equal(got[:nrays], want, "the host form against the device form")
    assert (got[nrays:] == PATTERN).all()                           # nothing behind the last ray's samples is written
    # what is never read: columns 0..3 and 9..11, [3] and [7] of the ray rows, the whole rows of Gaussians no ray keeps
    nan = np.float32(np.nan)
    table[:, :4] = nan
    table[:, 9:] = nan
    rows[:, 3] = nan
    rows[:, 7] = nan
    unkept = ~R.kept(sc.o, sc.d, sc.g).any(0)
    if name == "T small 5":
        assert unkept[1]                                            # the Gaussian of magnitude 0
    table[unkept] = nan
    got = device_call(renderer, case, s, table, rows, sd)
    np.testing.assert_array_equal(got[:nrays], want, "poison where nothing is read")
    assert (got[nrays:] == PATTERN).all()


def test_bits_no_table_is_a_table_of_zeros_and_reads_no_stale_one(renderer, oracle):
    """tangent = NULL means zero: the same bits as a table of zeros, also right behind a host call that staged a table of NaN."""
    case = T.case(oracle, "T grid16 scattered")
    sc = case.sc
    setup(renderer, sc.g)
    _, rv, sd = dense(case)
    want = run(renderer, case, case.s, None, rv, sd)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    poisoned = run(renderer, case, case.s, np.full((len(sc.g), 5), np.nan, np.float32), rv, sd)
    assert np.isnan(poisoned).any()
    np.testing.assert_array_equal(bits(run(renderer, case, case.s, None, rv, sd)), bits(want), "behind a staged table of NaN")
    np.testing.assert_array_equal(bits(run(renderer, case, case.s, np.zeros((len(sc.g), 5), np.float32), rv, sd)), bits(want), "a table of zeros")
    np.testing.assert_array_equal(bits(run(renderer, case, case.s, None, rv, np.zeros_like(sd))), bits(run(renderer, case, case.s, None, rv, None)),
                                  "sample tangents of zero")


# ---- zeros ----
@pytest.mark.parametrize("mode", ["T", "depth"])
def test_zeros(renderer, oracle, mode):
    base = T.case(oracle, f"{mode} small 5")
    bsc = base.sc
    # one more ray, far off and parallel to the scene: it keeps nothing
    o = np.concatenate([np.broadcast_to(bsc.o, bsc.d.shape), [[0.0, 50.0, 0.0]]]).astype(np.float32)
    d = np.concatenate([bsc.d, [[1.0, 0.0, 0.0]]]).astype(np.float32)
    sc = G.GradScene("small 5 and a miss", bsc.g, o, d, None, [])
    ns = base.ns
    rng = np.random.default_rng(3)
    for eps in T.EPS:
        assert not R.kept(o, d, sc.g, eps, 1)[-1].any() and R.kept(o, d, sc.g, eps, 1)[:-1].any(1).all()
        setup(renderer, sc.g, "vcl-as", eps)
        if mode == "T":
            s = np.concatenate([np.broadcast_to(base.s, base.g.shape), [np.linspace(0.5, 3.0, ns)]]).astype(np.float32)
        else:
            s = renderer.depth_bundle(o, d, np.concatenate([base.tau, np.full((1, ns), 0.5)]).astype(np.float32), True)
            s[-1] = 1.0                                             # a finite depth for the ray that keeps nothing: S_k == 0 there
        v, rv, sd = (rng.uniform(-1, 1, size=sh).astype(np.float32) for sh in ((len(sc.g), 5), (len(d), 6), s.shape))
        call = lambda *a: renderer.transmittance_bundle_tangent(o, d, s, *a, wrt=base.wrt, s_per_ray=True)
        zv, zr = np.zeros_like(TT.packed(v, len(sc.g))), np.zeros_like(TT.packed_rays(rv, len(d)))
        assert (call(zv, None, None) == 0).all() and (call(None, zr, None) == 0).all() and (call(zv, zr, np.zeros_like(sd)) == 0).all()
        got = call(TT.packed(v, len(sc.g)), TT.packed_rays(rv, len(d)), sd)
        assert (got[-1] == 0).all() and np.isfinite(got).all() and (got[:-1] != 0).any()       # the ray that keeps nothing: zeros, stored


# ---- refusals ----
def test_refusals(renderer, oracle, pkg):
    import torch
    case = T.case(oracle, "T small 5")
    sc = case.sc
    v, rv, sd = dense(case)
    nrays, ns = case.g.shape
    table, rows = TT.packed(v, len(sc.g)), TT.packed_rays(rv, nrays)
    s_rays = np.ascontiguousarray(np.broadcast_to(case.s, case.g.shape), np.float32)
    t_o, t_d, t_s, t_t, t_r, t_sd = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (sc.o, sc.d, s_rays, table, rows, sd))
    t_out = torch.from_numpy(np.full((nrays, ns), PATTERN, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    L, h = renderer._L, renderer._h
    f32p = C.POINTER(C.c_float)
    o, d = (np.ascontiguousarray(a, np.float32) for a in (sc.o, sc.d))
    out = np.full((nrays, ns), -1.0, np.float32)
    hp = dict(zip("o d s t r sd out".split(), (a.ctypes.data_as(f32p) for a in (o, d, s_rays, table, rows, sd, out))))
    dp = dict(zip("o d s t r sd out".split(), (t.data_ptr() for t in (t_o, t_d, t_s, t_t, t_r, t_sd, t_out))))

    def dev(**kw):
        a = {**dp, **dict(ctx=h, n=nrays, ns=ns, spr=1, wrt=TGRAD_T), **kw}
        return L.vrt_hip_transmittance_bundle_tangent_device(a["ctx"], a["n"], a["o"], 0, a["d"], a["s"], a["ns"], a["spr"], a["wrt"], a["t"], a["r"], a["sd"], 1,
                                                             a["out"], None)

    def host(**kw):
        a = {**hp, **dict(n=nrays, ns=ns, spr=1, wrt=TGRAD_T), **kw}
        return L.vrt_hip_transmittance_bundle_tangent(h, a["n"], a["o"], 0, a["d"], a["s"], a["ns"], a["spr"], a["wrt"], a["t"], a["r"], a["sd"], 1, a["out"])

    def message(text):
        assert text in L.vrt_hip_last_error(h), (text, L.vrt_hip_last_error(h))
    try:
        setup(renderer, sc.g)
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_SPLINE, 1e-9)                      # a pair with jumps
        assert dev() == -1
        message(b"transmittance_bundle_tangent")
        assert host() == -1
        with pytest.raises(pkg.VrtHipError):
            renderer.transmittance_bundle_tangent(sc.o, sc.d, case.s, table, rows, sd)
        setup(renderer, sc.g)                                                          # a supported pair again
        for null in ("o", "d", "s", "out"):
            assert dev(**{null: None}) == -1 and host(**{null: None}) == -1, null
            message(b"NULL")
        assert dev(t=None, r=None, sd=None) == -1 and host(t=None, r=None, sd=None) == -1      # all three inputs NULL
        message(b"none of a tangent table, ray tangents and sample tangents")
        for wrt in (-1, 2):
            assert dev(wrt=wrt) == -1 and host(wrt=wrt) == -1
            message(b"wrt")
        assert dev(wrt=TGRAD_DEPTH, spr=0) == -1 and host(wrt=TGRAD_DEPTH, spr=0) == -1      # depth mode takes a depth per ray
        message(b"depth mode")
        assert dev(n=2 ** 32) == -1
        message(b"2^32")
        assert dev(ns=2 ** 62) == -1
        message(b"does not fit")
        assert dev(ctx=None) == -1
        # nothing to do: no rays, no samples, NULLs allowed
        nulls = dict(o=None, d=None, s=None, t=None, r=None, sd=None, out=None)
        assert dev(n=0, **nulls) == 0 and host(n=0, **nulls) == 0
        assert dev(ns=0, s=None, sd=None, out=None) == 0 and host(ns=0, s=None, sd=None, out=None) == 0
        renderer.set_gaussians(sc.g[:0])                                               # a scene of no Gaussians
        assert dev() == 0 and host() == 0
        renderer.sync()
        torch.cuda.synchronize()
        assert (bits(t_out.cpu().numpy()) == PATTERN).all() and (out == -1.0).all()   # nothing was enqueued, nothing written
    finally:
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        renderer.set_gaussians(sc.g)


# ---- statistics ----
@pytest.mark.parametrize("name", ["T grid16 scattered", f"depth wide {RAY_LCAP + 1}"])
def test_statistics_are_the_radiance_bundles(renderer, oracle, name):
    case = T.case(oracle, name)
    sc = case.sc
    setup(renderer, sc.g)
    s = device_samples(renderer, case)
    v, rv, sd = dense(case)
    renderer.enable_stats(True)
    try:
        for index in (0, 1):
            renderer.set_ray_index(index)
            renderer.radiance_rays(sc.o, sc.d)
            want, want_index = renderer.ray_stats(), renderer.ray_index_stats()
            run(renderer, case, s, v, rv, sd)
            assert renderer.ray_stats() == want and want["rays"] == len(sc.d), (name, index)
            assert renderer.ray_index_stats() == want_index and want_index["indexed"] == index, (name, index)
    finally:
        renderer.set_ray_index(0)
        renderer.enable_stats(False)


# ---- torch: forward-mode AD of autograd.transmittance_bundle and autograd.depth_bundle ----
def tensors(sc, requires_grad=False):
    import torch
    p = G.params64(sc.g)
    return [torch.tensor(p[k], dtype=torch.float32, device="cuda", requires_grad=requires_grad) for k in ("mu", "albedo", "sigma", "magnitude")]


def split(v):
    """v [N, 5] as the tangents of (mu, albedo, sigma, magnitude); the albedo's moves nothing"""
    import torch
    alb = np.random.default_rng(2).uniform(-1, 1, size=(len(v), 4)).astype(np.float32)
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (v[:, 0:3], alb, v[:, 3], v[:, 4])]


def profile_fn(mode):
    from sgrt_amd import autograd
    return autograd.transmittance_bundle if mode == "T" else autograd.depth_bundle


def values_of(case):
    return case.s if case.wrt == TGRAD_T else case.tau


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_func_jvp_gives_the_direct_calls_bits(renderer, oracle, mode):
    import torch
    case = T.case(oracle, f"{mode} small 9")
    sc = case.sc
    s, want = dense_run(renderer, case)
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    v, rv, sd = dense(case)
    fn = profile_fn(mode)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    t_o, t_d = cuda(sc.o), cuda(sc.d)
    # one origin for the bundle: its tangent is one row -- the dense direction's rows differ, so the origin goes per ray; the values go
    # per ray as well, the dense direction's sample tangents differ from ray to ray
    o_rays = t_o.reshape(1, 3).expand(len(sc.d), 3).contiguous()
    vals = cuda(np.broadcast_to(values_of(case), case.g.shape))
    tangents = (*split(v), cuda(rv[:, :3]), cuda(rv[:, 3:]), cuda(sd))
    out, Jv = torch.func.jvp(lambda *a: fn(renderer, *a), (*tensors(sc), o_rays, t_d, vals), tangents)
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(s if mode == "depth" else renderer.transmittance_bundle(sc.o, sc.d, case.s)))
    np.testing.assert_array_equal(bits(Jv.cpu().numpy()), bits(want))
    # a [3] origin: its tangent moves every ray's origin alike
    shared = next(x[2] for x in TT.directions(case) if x[0] == "origin shared")
    _, Jv = torch.func.jvp(lambda o: fn(renderer, *tensors(sc), o, t_d, cuda(values_of(case))), (t_o,), (cuda(shared[0, :3]),))
    setup(renderer, sc.g)
    np.testing.assert_array_equal(bits(Jv.cpu().numpy()), bits(run(renderer, case, s, None, shared, None)))


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_func_jvp_with_values_shared_by_the_rays(renderer, oracle, mode):
    """s [ns] or tau [nt] for every ray: the tangent has their shape and broadcasts as they do"""
    import torch
    case = T.case(oracle, "T small 2" if mode == "T" else "depth small 9")
    sc = case.sc
    shared_values = case.s if mode == "T" else np.ascontiguousarray(case.tau[0])
    assert shared_values.ndim == 1
    shared_sd = next(x[3] for x in TT.directions(case) if x[0] == "samples shared")
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    fn = profile_fn(mode)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    t_o, t_d = cuda(sc.o), cuda(sc.d)
    out, Jv = torch.func.jvp(lambda x: fn(renderer, *tensors(sc), t_o, t_d, x), (cuda(shared_values),), (cuda(shared_sd),))
    setup(renderer, sc.g)
    s = shared_values if mode == "T" else out.cpu().numpy()
    assert np.abs(Jv.cpu().numpy()).max() > 0
    np.testing.assert_array_equal(bits(Jv.cpu().numpy()), bits(run(renderer, case, s, None, None, shared_sd)))


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_forward_ad_passes_only_what_has_a_tangent(renderer, oracle, monkeypatch, mode):
    import torch
    import torch.autograd.forward_ad as fwAD
    case = T.case(oracle, f"{mode} small 5")
    sc = case.sc
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    v, rv, sd = dense(case)
    fn = profile_fn(mode)
    calls = []
    real = renderer.transmittance_bundle_tangent_device

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(renderer, "transmittance_bundle_tangent_device", spy)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    t_o, t_d, vals = cuda(sc.o), cuda(sc.d), cuda(np.broadcast_to(values_of(case), case.g.shape))
    with fwAD.dual_level():
        dual = fwAD.make_dual(t_d, cuda(rv[:, 3:]))
        Jd = fwAD.unpack_dual(fn(renderer, *tensors(sc), t_o, dual, vals)).tangent
        assert len(calls) == 1 and calls[0]["d_tangent"] == 0 and calls[0]["d_ray_tangent"] != 0 and calls[0]["d_s_tangent"] == 0      # rays alone
        dual = fwAD.make_dual(vals, cuda(sd))
        Js = fwAD.unpack_dual(fn(renderer, *tensors(sc), t_o, t_d, dual)).tangent
        assert len(calls) == 2 and calls[1]["d_tangent"] == 0 and calls[1]["d_ray_tangent"] == 0 and calls[1]["d_s_tangent"] != 0      # samples alone
        ps = tensors(sc)
        ps[2] = fwAD.make_dual(ps[2], cuda(v[:, 3]))
        Jg = fwAD.unpack_dual(fn(renderer, *ps, t_o, t_d, vals)).tangent
        assert len(calls) == 3 and calls[2]["d_tangent"] != 0 and calls[2]["d_ray_tangent"] == 0 and calls[2]["d_s_tangent"] == 0      # the table alone
        ps = tensors(sc)
        ps[1] = fwAD.make_dual(ps[1], torch.ones_like(ps[1]))
        Ja = fwAD.unpack_dual(fn(renderer, *ps, t_o, t_d, vals)).tangent
        assert len(calls) == 3 and (Ja is None or not Ja.any())                                          # albedo alone moves nothing: nothing issued
        fn(renderer, *tensors(sc), t_o, t_d, vals)
        assert len(calls) == 3                                                                          # no tangent anywhere: nothing issued
    setup(renderer, sc.g)
    s = device_samples(renderer, case)
    s = np.ascontiguousarray(np.broadcast_to(s, case.g.shape))
    only_dirs, only_sigma = np.zeros_like(rv), np.zeros_like(v)
    only_dirs[:, 3:], only_sigma[:, 3] = rv[:, 3:], v[:, 3]
    np.testing.assert_array_equal(bits(Jd.cpu().numpy()), bits(run(renderer, case, s, None, only_dirs, None)))
    np.testing.assert_array_equal(bits(Js.cpu().numpy()), bits(run(renderer, case, s, None, None, sd)))
    np.testing.assert_array_equal(bits(Jg.cpu().numpy()), bits(run(renderer, case, s, only_sigma, None, None)))


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_backward_still_gives_what_it_gave(renderer, oracle, mode):
    """backward after the move to forward / setup_context: the ray rows and the values' gradient are the binding's bits (no atomic add
    takes part in them), the parameters' gradients the binding's table within two bounds -- and a jvp in between changes neither."""
    import torch
    case = T.case(oracle, f"{mode} small 9")
    sc = case.sc
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    fn = profile_fn(mode)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    ps = tensors(sc, requires_grad=True)
    o_rays = cuda(np.broadcast_to(sc.o, sc.d.shape)).requires_grad_(True)
    t_d = cuda(sc.d).requires_grad_(True)
    vals = cuda(values_of(case)).requires_grad_(True)
    out = fn(renderer, *ps, o_rays, t_d, vals)
    fwd = out.detach().cpu().numpy()
    live = np.isfinite(fwd)
    g = np.where(live, case.g, 0.0).astype(np.float32)
    torch.func.jvp(lambda x: fn(renderer, *tensors(sc), o_rays.detach(), x, vals.detach()), (t_d.detach(),), (torch.ones_like(t_d),))
    torch.where(cuda(live).bool(), out * cuda(g), torch.zeros_like(out)).sum().backward()
    assert ps[1].grad is None
    setup(renderer, sc.g)
    s = case.s if mode == "T" else fwd
    o, d = rays_of(case)
    table, gs, rows = renderer.transmittance_bundle_grad(o, d, s, g, wrt=case.wrt, s_per_ray=s.ndim == 2, want_rays=True)
    np.testing.assert_array_equal(bits(o_rays.grad.cpu().numpy()), bits(rows["origin"]))
    np.testing.assert_array_equal(bits(t_d.grad.cpu().numpy()), bits(rows["dir"]))
    if vals.dim() == 2:
        np.testing.assert_array_equal(bits(vals.grad.cpu().numpy()), bits(gs))
    m = T.bundle_tgrad(case, "vcl-as", 1e-9, s=s, g=g)
    got = T.table_of({"mu": ps[0].grad.cpu().numpy(), "sigma": ps[2].grad.cpu().numpy(), "magnitude": ps[3].grad.cpu().numpy()})
    assert (np.abs(got - T.table_of(table)) <= 2 * T.bound(m.S)).all()
