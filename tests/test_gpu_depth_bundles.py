"""Depth bundles on the GPU (vrt_hip_depth_bundle*, csrc/vrt_ray_depth_kernel.hip): the distance along any rays at which the
transmittance falls to a level, culled per ray like the other two kinds of bundle.  Scenes, levels, the float64 model and the
acceptance rules are tests/depth_bundle_scenes.py's; tests/test_depth_bundle_scenes.py shows on the CPU that they see what they are
meant to see.  The oracle is oracle.transmittance per ray over the WHOLE scene with the float32 origins and directions the GPU gets.

A finite result s* is accepted when the oracle brackets the level within delta = 4 max(ulp32(s*), s_end 2^-24) of it, up to the
transmittance bundles' own tolerance in T, and where the model's slope is above 0.05 s* is within delta + tol_T / slope of the
float64 root; +inf is demanded where the model's T_inf is above the level by more than tol_T, a finite result where it is below.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_bundle_scenes as S
from conftest import ROOT
from depth_bundle_scenes import RAY_PL, RAY_LCAP, TOL, SG

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "simd-gaussian-ray-tracing_amd", "bin")
PAIRS = {"vcl-as": (1, 1), "libm-libm": (0, 0)}     # (Exp, Erf): the same numbers in the package and in the oracle
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def grid(oracle, dim):
    return cached(("grid", dim), lambda: oracle.grid_scene(dim))


def bundle(oracle, name, dim=16):
    g = grid(oracle, dim)
    return cached((name, dim), lambda: S.coherent_rays(g) if name == "coherent" else S.scattered_rays(g))


def model_of(key, o, d, g, pair=(1, 1)):
    """({ray: RayModel with the pair's Erf}, tol_T per ray): computed once per (scene, rays, Erf) and shared, unchanged, among the tests."""
    return cached(("model", key, pair[1]), lambda: (S.models(o, d, g, erf_kind=pair[1]), S.ray_tolerances(o, d, g)))


def setup(renderer, g, pair=(1, 1), eps=1e-9):
    renderer.set_gaussians(g)
    renderer.set_options(pair[0], pair[1], eps)
    renderer.clear_tiles()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def accept(oracle, what, o, d, g, depth, levels, mods, tol_T, pair=(1, 1), rays=None):
    """The finite-result and the miss acceptance over the rays of `mods` (or `rays` of them); returns the number of finite results."""
    levels = np.asarray(levels, np.float32)
    rays = list(mods) if rays is None else rays
    sub = {r: mods[r] for r in rays}
    excluded = S.check_misses(depth, sub, levels, tol_T, what)
    worst, nfinite = 0.0, 0
    for r in rays:
        lv = levels[r] if levels.ndim == 2 else levels
        for k, tau in enumerate(lv):
            if np.isfinite(depth[r, k]):
                _, off, bound = S.check_finite(oracle, o, d, g, r, depth[r, k], tau, float(tol_T[r]), mods[r], pair, what)
                nfinite += 1
                if off is not None:
                    worst = max(worst, off / bound)
    print(f"{what}: {nfinite} finite results of {len(rays) * levels.shape[-1]}, excluded from the miss check {excluded:.1%}, "
          f"largest |s* - s64| / bound {worst:.3f}")
    return nfinite


def postcondition(renderer, o, d, depth, levels, what):
    """(4., called by 1. - 3.)  T(depth) through a transmittance bundle on the same context is at or below the level, exactly, for every finite result."""
    levels = np.broadcast_to(np.asarray(levels, np.float32), depth.shape)
    fin = np.isfinite(depth)
    T = renderer.transmittance_bundle(o, d, np.ascontiguousarray(np.where(fin, depth, 0.0).astype(np.float32)), s_per_ray=True)
    assert fin.any() and (T[fin] <= levels[fin]).all(), (what, float((T[fin] - levels[fin]).max()))


# ---- 1. parity ----
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("name", ["coherent", "scattered"])
def test_parity_grid16(renderer, oracle, name, pair):
    ex = PAIRS[pair]
    g = grid(oracle, 16)
    o, d = bundle(oracle, name)
    assert (o.size == 3) == (name == "coherent") and len(d) == (130 if name == "coherent" else 32)
    mods, tol_T = model_of(name, o, d, g, ex)
    setup(renderer, g, ex)
    shared = renderer.depth_bundle(o, d, S.PARITY_LEVELS)
    assert shared.shape == (len(d), len(S.PARITY_LEVELS))
    assert accept(oracle, f"{name} {pair}", o, d, g, shared, S.PARITY_LEVELS, mods, tol_T, ex) >= 30
    per_ray = S.per_ray_levels(S.PARITY_LEVELS, len(d))
    own = renderer.depth_bundle(o, d, per_ray)
    accept(oracle, f"{name} {pair} per ray", o, d, g, own, per_ray, mods, tol_T, ex)
    order = np.argsort(-per_ray, axis=1, kind="stable")         # back into the shared order: the same bits
    np.testing.assert_array_equal(bits(np.take_along_axis(own, order, 1)), bits(shared))
    postcondition(renderer, o, d, shared, S.PARITY_LEVELS, f"{name} {pair}")


# ---- 2. RAY_PL ----
def stack_levels():
    return np.concatenate([S.STACK_LEVELS, S.STACK_MARKER_LEVELS, [S.STACK_MISS_LEVEL]]).astype(np.float32)


def stack_scene(oracle, k):
    at, over = S.one_over_pair(oracle)
    return {RAY_PL - 1: lambda: S.stack_with_side(oracle, RAY_PL - 1), RAY_PL: lambda: at, RAY_PL + 1: lambda: over}[k]()


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("k, long_rays", [(RAY_PL - 1, 0), (RAY_PL, 0), (RAY_PL + 1, 2)])
def test_list_capacity(renderer, oracle, k, long_rays, pair):
    ex = PAIRS[pair]
    g = stack_scene(oracle, k)
    o, d = S.stack_rays()
    levels = stack_levels()
    mods, tol_T = model_of(("stack", k), o, d, g, ex)
    setup(renderer, g, ex)
    renderer.enable_stats(True)
    try:
        depth = renderer.depth_bundle(o, d, levels)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    assert st["rays"] == 64 and st["long_rays"] == long_rays and st["short_rays"] == 64 - long_rays
    assert (tol_T[:2] == (S.TOL_FULL_SUM + S.cull_bound(len(g)) if k <= RAY_PL else TOL)).all()
    accept(oracle, f"stack {k} {pair}", o, d, g, depth, levels, mods, tol_T, ex)
    nl = len(S.STACK_LEVELS)
    assert np.isfinite(depth[:2, :nl]).all() and np.isfinite(depth[0, nl]) and np.isfinite(depth[1, nl + 1])     # the marker levels
    assert np.isinf(depth[:2, -1]).all()                        # the axial rays stay above 0.1
    free = [r for r in range(2, 64) if len(mods[r].w) == 0]
    assert len(free) >= 40 and np.isinf(depth[free]).all() and (depth[free] > 0).all()     # wave-mates that keep nothing
    assert np.isfinite(depth[2, 0])                             # ... and one with a depth of its own, behind the side column
    postcondition(renderer, o, d, depth, levels, f"stack {k} {pair}")


def test_one_lane_over_the_limit_does_not_move_its_wave_mates(renderer, oracle):
    at, over = S.one_over_pair(oracle)
    o, d = S.stack_rays()
    levels = stack_levels()
    res = []
    for g in (at, over):
        setup(renderer, g)
        res.append(renderer.depth_bundle(o, d, levels))
    np.testing.assert_array_equal(bits(res[0][2:]), bits(res[1][2:]))
    assert np.isfinite(res[0][2:]).any()
    nl = len(S.STACK_LEVELS)                                    # the extra Gaussian is the last of the stack: seen at the marker levels
    assert np.isfinite([res[k][r, nl + r] for k in (0, 1) for r in (0, 1)]).all()
    assert res[0][0, nl] - res[1][0, nl] >= 5e-3 and res[0][1, nl + 1] - res[1][1, nl + 1] >= 5e-3


# ---- 3. RAY_LCAP ----
def wide_levels():
    return np.concatenate([S.WIDE_LEVELS, [S.WIDE_MARKER_LEVEL, S.WIDE_MISS_LEVEL]]).astype(np.float32)


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("n, scratch_rays", [(RAY_LCAP - 1, 0), (RAY_LCAP, 0), (RAY_LCAP + 1, 1)])
def test_lds_capacity_of_the_long_kernel(renderer, oracle, n, scratch_rays, pair):
    ex = PAIRS[pair]
    sc = S.wide_stack(oracle, RAY_LCAP, n)
    o, d = S.wide_rays()
    levels = wide_levels()
    mods, tol_T = model_of(("wide", n), o, d, sc.g, ex)
    assert (tol_T == TOL).all()
    setup(renderer, sc.g, ex)
    depth = renderer.depth_bundle(o, d, levels)
    assert accept(oracle, f"wide stack {n} {pair}", o, d, sc.g, depth, levels, mods, tol_T, ex) == 9
    assert np.isinf(depth[:, -1]).all()
    renderer.enable_stats(True)
    try:
        one = renderer.depth_bundle(o, d[:1], levels)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    assert st["long_rays"] == 1 and st["scratch_rays"] == scratch_rays
    np.testing.assert_array_equal(bits(one[0]), bits(depth[0]))
    postcondition(renderer, o, d, depth, levels, f"wide stack {n} {pair}")


# ---- 5. the level loop ----
@pytest.mark.parametrize("per_ray", [False, True])
def test_level_groups(renderer, oracle, per_ray):
    """Short and long rays in one wave; every depth[r, k] is what an nt = 1 call with that single level returns, bit for bit."""
    g = S.stack_with_side(oracle, RAY_PL + 1)
    o, d = S.stack_rays()
    setup(renderer, g)
    rng = np.random.default_rng(17)
    nmax = 2 * SG + 1
    lv = (rng.uniform(0.05, 1.0, size=(len(d), nmax)) if per_ray else np.tile(np.linspace(0.97, 0.12, nmax), (len(d), 1))).astype(np.float32)
    lv[:, -1] = 0.08                                                # below every ray's T_inf
    single = np.stack([renderer.depth_bundle(o, d, np.ascontiguousarray(lv[:, k:k + 1]) if per_ray else lv[0, k:k + 1],
                                             tau_per_ray=per_ray)[:, 0] for k in range(nmax)], 1)
    assert np.isfinite(single[:2]).any() and np.isinf(single[:2]).any() and np.isfinite(single[2:]).any() and np.isinf(single[2:]).any()
    for nt in (1, SG - 1, SG, SG + 1, 2 * SG + 1):
        tau = np.ascontiguousarray(lv[:, :nt]) if per_ray else lv[0, :nt]
        depth = renderer.depth_bundle(o, d, tau, tau_per_ray=per_ray)
        assert depth.shape == (len(d), nt)
        np.testing.assert_array_equal(bits(depth), bits(single[:, :nt]), err_msg=f"nt = {nt}")
    if not per_ray:                                                 # shared levels == those levels per ray
        np.testing.assert_array_equal(bits(renderer.depth_bundle(o, d, np.ascontiguousarray(lv[:, :SG + 1]), tau_per_ray=True)), bits(single[:, :SG + 1]))


# ---- 6. bundle independence ----
@pytest.mark.parametrize("nrays", [1, 63, 64, 65])
def test_bundle_sizes(renderer, oracle, nrays):
    g = grid(oracle, 16)
    o, d = bundle(oracle, "coherent")
    setup(renderer, g)
    whole = cached("coherent gpu", lambda: renderer.depth_bundle(o, d, S.PARITY_LEVELS))
    depth = renderer.depth_bundle(o, d[:nrays], S.PARITY_LEVELS)
    assert depth.shape == (nrays, len(S.PARITY_LEVELS)) and np.isfinite(whole[:, 0]).any()
    np.testing.assert_array_equal(bits(depth), bits(whole[:nrays]))


def test_a_permuted_bundle_gives_the_permuted_result(renderer, oracle):
    g = grid(oracle, 16)
    setup(renderer, g)
    o, d = bundle(oracle, "scattered")
    depth = renderer.depth_bundle(o, d, S.PARITY_LEVELS)
    perm = np.random.default_rng(1).permutation(len(d))
    np.testing.assert_array_equal(bits(renderer.depth_bundle(o[perm], d[perm], S.PARITY_LEVELS)), bits(depth[perm]))
    own = S.per_ray_levels(S.PARITY_LEVELS, len(d))
    d2 = renderer.depth_bundle(o, d, own)
    np.testing.assert_array_equal(bits(renderer.depth_bundle(o[perm], d[perm], np.ascontiguousarray(own[perm]))), bits(d2[perm]))
    oc, dc = bundle(oracle, "coherent")
    one = renderer.depth_bundle(oc, dc, S.PARITY_LEVELS)
    np.testing.assert_array_equal(bits(renderer.depth_bundle(np.tile(oc, (len(dc), 1)), dc, S.PARITY_LEVELS)), bits(one))   # one origin == that origin per ray


# ---- 7. monotony and ends ----
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_monotony_and_ends(renderer, oracle, pair):
    ex = PAIRS[pair]
    levels = np.array([1.5, 1.0, 0.999, 0.9, 0.7, 0.5, 0.3, 0.2, 0.14, 0.1, 0.0, -1.0], np.float32)     # descending
    for what, g, (o, d) in (("stack 33", S.stack_with_side(oracle, RAY_PL + 1), S.stack_rays()), ("grid16", grid(oracle, 16), bundle(oracle, "scattered"))):
        setup(renderer, g, ex)
        depth = renderer.depth_bundle(o, d, levels)
        assert not np.isnan(depth).any()
        assert (depth[:, 1:] >= depth[:, :-1]).all(), what      # a lower level lies deeper; a ray never comes back from +inf
        assert (depth[:, :2] == 0).all() and (np.signbit(depth[:, :2]) == 0).all(), what
        assert np.isinf(depth[:, -2:]).all() and (depth[:, -2:] > 0).all(), what
        assert np.isfinite(depth[:, 3]).any() and (depth[:, 2:] > 0).all(), what
        with_nan = levels.copy()
        with_nan[[1, 5]] = np.nan
        dn = renderer.depth_bundle(o, d, with_nan)
        assert np.isnan(dn[:, [1, 5]]).all(), what
        keep = [k for k in range(len(levels)) if k not in (1, 5)]
        np.testing.assert_array_equal(bits(dn[:, keep]), bits(depth[:, keep]), err_msg=what)
    o, d = bundle(oracle, "scattered")
    setup(renderer, grid(oracle, 16)[:0], ex)                   # no Gaussians at all
    depth = renderer.depth_bundle(o, d, np.array([1.5, 1.0, 0.999, 0.5, 0.0, -1.0], np.float32))
    assert (depth[:, :2] == 0).all() and np.isinf(depth[:, 2:]).all() and (depth[:, 2:] > 0).all()


# ---- 8. index on = off, and the same cull as radiance ----
def index_cases(oracle):
    g16 = grid(oracle, 16)
    at, over = S.one_over_pair(oracle)
    cases = [("grid16 coherent", g16) + bundle(oracle, "coherent") + (S.PARITY_LEVELS,),
             ("grid16 scattered", g16) + bundle(oracle, "scattered") + (S.PARITY_LEVELS,),
             ("stack 31", S.stack_with_side(oracle, RAY_PL - 1)) + S.stack_rays() + (stack_levels(),),
             ("stack 32", at) + S.stack_rays() + (stack_levels(),), ("stack 33", over) + S.stack_rays() + (stack_levels(),)]
    return cases + [(f"wide {n}", S.wide_stack(oracle, RAY_LCAP, n).g) + S.wide_rays() + (wide_levels(),) for n in (RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1)]


def test_index_on_equals_index_off(renderer, oracle):
    try:
        for name, g, o, d, levels in index_cases(oracle):
            setup(renderer, g)
            renderer.set_ray_index(0)
            off = renderer.depth_bundle(o, d, levels)
            renderer.set_ray_index(1)
            on = renderer.depth_bundle(o, d, levels)
            assert np.isfinite(off).any() and np.isinf(off).any(), name
            np.testing.assert_array_equal(bits(on), bits(off), err_msg=name)
    finally:
        renderer.set_ray_index(0)


@pytest.mark.parametrize("index", [0, 1])
def test_same_cull_as_radiance(renderer, oracle, index):
    renderer.enable_stats(True)
    try:
        for name, g, o, d, levels in index_cases(oracle):
            setup(renderer, g)
            renderer.set_ray_index(index)
            renderer.radiance_rays(o, d)
            want, want_index = renderer.ray_stats(), renderer.ray_index_stats()
            renderer.depth_bundle(o, d, levels)
            got, got_index = renderer.ray_stats(), renderer.ray_index_stats()
            assert want["rays"] == len(d) and got == want, name
            assert got_index == want_index and got_index["indexed"] == index, name
    finally:
        renderer.set_ray_index(0)
        renderer.enable_stats(False)


# ---- device form ----
def test_device_form_on_a_callers_stream(renderer, oracle):
    import torch
    g = grid(oracle, 16)
    setup(renderer, g)
    o, d = bundle(oracle, "scattered")
    want = renderer.depth_bundle(o, d, S.PARITY_LEVELS)
    own = S.per_ray_levels(S.PARITY_LEVELS, len(d))
    want2 = renderer.depth_bundle(o, d, own)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t_o, t_d, t_l, t_l2 = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o, d, S.PARITY_LEVELS, own))
        t_D = torch.full(want.shape, -1.0, dtype=torch.float32, device="cuda")
        t_D2 = torch.full(want2.shape, -1.0, dtype=torch.float32, device="cuda")
        st.synchronize()
        renderer.depth_bundle_device(len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_l.data_ptr(), len(S.PARITY_LEVELS), 0, t_D.data_ptr(), stream=st.cuda_stream)
        free_before = torch.cuda.mem_get_info()[0]
        renderer.depth_bundle_device(len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_l2.data_ptr(), own.shape[1], 1, t_D2.data_ptr(), stream=st.cuda_stream)
        free_after = torch.cuda.mem_get_info()[0]                    # the second call of the same size: no allocation
        st.synchronize()
    np.testing.assert_array_equal(bits(t_D.cpu().numpy()), bits(want))
    np.testing.assert_array_equal(bits(t_D2.cpu().numpy()), bits(want2))
    assert free_after == free_before


# ---- 9. refusals and no-ops ----
def test_argument_errors(renderer, oracle, pkg):
    import torch
    setup(renderer, grid(oracle, 16))
    o, d = bundle(oracle, "scattered")
    lv = S.PARITY_LEVELS
    L, f32p = pkg.lib(), C.POINTER(C.c_float)
    D = np.full((len(d), len(lv)), -1.0, np.float32)
    op, dp, lp, Dp = o.ctypes.data_as(f32p), d.ctypes.data_as(f32p), lv.ctypes.data_as(f32p), D.ctypes.data_as(f32p)
    host = L.vrt_hip_depth_bundle
    assert host(renderer._h, len(d), op, 1, None, lp, len(lv), 0, Dp) == -1      # VRT_HIP_ERR_INVALID
    assert host(renderer._h, len(d), None, 1, dp, lp, len(lv), 0, Dp) == -1
    assert host(renderer._h, len(d), op, 1, dp, None, len(lv), 0, Dp) == -1
    assert host(renderer._h, len(d), op, 1, dp, lp, len(lv), 0, None) == -1
    assert host(None, len(d), op, 1, dp, lp, len(lv), 0, Dp) == -1
    assert host(renderer._h, 2 ** 32, op, 1, dp, lp, len(lv), 0, Dp) == -1         # more rays than the u32 queue holds
    assert host(renderer._h, len(d), op, 1, dp, lp, 2 ** 62, 0, Dp) == -1          # nrays * nt does not fit
    assert (D == -1.0).all()
    assert host(renderer._h, 0, None, 1, None, None, len(lv), 0, None) == 0         # nothing to do
    assert host(renderer._h, len(d), None, 1, None, None, 0, 0, None) == 0
    t_o, t_d, t_l = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o, d, lv))
    t_D = torch.full(D.shape, -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev = L.vrt_hip_depth_bundle_device
    assert dev(renderer._h, len(d), t_o.data_ptr(), 1, None, t_l.data_ptr(), len(lv), 0, t_D.data_ptr(), None) == -1
    assert dev(renderer._h, len(d), None, 1, t_d.data_ptr(), t_l.data_ptr(), len(lv), 0, t_D.data_ptr(), None) == -1
    assert dev(renderer._h, len(d), t_o.data_ptr(), 1, t_d.data_ptr(), None, len(lv), 0, t_D.data_ptr(), None) == -1
    assert dev(renderer._h, len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_l.data_ptr(), len(lv), 0, None, None) == -1
    assert dev(renderer._h, 2 ** 32, t_o.data_ptr(), 1, t_d.data_ptr(), t_l.data_ptr(), len(lv), 0, t_D.data_ptr(), None) == -1
    assert dev(renderer._h, len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_l.data_ptr(), 2 ** 62, 0, t_D.data_ptr(), None) == -1
    assert dev(renderer._h, 0, None, 1, None, None, len(lv), 0, None, None) == 0
    assert dev(renderer._h, len(d), None, 1, None, None, 0, 0, None, None) == 0
    renderer.sync()
    torch.cuda.synchronize()
    assert (t_D.cpu().numpy() == -1.0).all()                         # nothing was enqueued
    with pytest.raises(pkg.VrtHipError):
        renderer.depth_bundle_device(len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_l.data_ptr(), len(lv), 0, 0)
    assert renderer.depth_bundle(np.zeros(3, np.float32), np.zeros((0, 3), np.float32), lv).shape == (0, len(lv))


# ---- the C++ example ----
def test_cpp_first_hit_example(renderer, oracle):
    """host/first_hit_example.cpp (vrt::radiance_rays, vrt::depth_bundle at tau = 0.5, shadow rays from the hits through
    vrt::transmittance_bundle): what it prints is what the Python binding gives for the same rays."""
    p = subprocess.run([os.path.join(BIN, "first_hit_example")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    num = r"[-+0-9.e]+|inf|nan"
    f3, head = rf"((?:(?:{num}) ){{3}})", rf"ray (\d+) o ((?:(?:{num}) ){{3}})n ((?:(?:{num}) ){{3}})L ((?:(?:{num}) ){{4}})depth ({num})"
    rows = [re.fullmatch(head + rf"(?: hit {f3}to_light {f3}dist ({num}) T ({num}))?", ln) for ln in p.stdout.strip().splitlines()]
    assert len(rows) == 12 and all(rows), p.stdout
    vec = lambda k, rs: np.array([[float(v) for v in m.group(k).split()] for m in rs], np.float32)  # noqa: E731
    o, d, L, depth = vec(2, rows), vec(3, rows), vec(4, rows), vec(5, rows)[:, 0]
    g = oracle.gaussians([[0, 1, 0, .1], [0, 0, 1, .7], [1, 0, 0, 1]], [[.3, .3, .5], [-.3, -.3, 0], [0, 0, 2]], [0.1, 0.4, 0.75], [2, .7, 1])
    setup(renderer, g)
    np.testing.assert_array_equal(bits(renderer.depth_bundle(o, d, np.array([0.5], np.float32))[:, 0]), bits(depth))
    np.testing.assert_array_equal(bits(renderer.radiance_rays(o, d)), bits(L))
    hits = [m for m in rows if m.group(6)]
    assert [bool(m.group(6)) for m in rows] == list(np.isfinite(depth)) and 2 <= len(hits) < 12
    so, sn, dist, T = vec(6, hits), vec(7, hits), vec(8, hits)[:, 0], vec(9, hits)[:, 0]
    np.testing.assert_array_equal(bits(renderer.transmittance_bundle(so, sn, dist.reshape(-1, 1))[:, 0]), bits(T))
    assert np.abs(so - (o[np.isfinite(depth)] + d[np.isfinite(depth)] * depth[np.isfinite(depth), None])).max() <= 1e-5
    assert T.min() < 0.99 and T.max() <= 1.0                        # some of the light is lost on the way out
