"""Transmittance bundles on the GPU (vrt_hip_transmittance_bundle*, csrc/vrt_ray_trans_kernel.hip): T at several depths of any rays,
culled per ray like the radiance bundles.  The oracle is always oracle.transmittance per ray over the WHOLE scene with the float32
origins, directions and samples the GPU gets; tests/test_transmittance_bundle_scenes.py shows on the CPU that the scenes and samples
of tests/transmittance_bundle_scenes.py see what they are meant to.

Tolerances (transmittance_bundle_scenes.tolerance): 2e-6 + 0.8 cull_eps min(N, 4096) for a ray the lane = ray kernel sums for certain
(the full sum's 2e-6 of test_gpu_parity.py plus the cull bound), TOL = 1e-4 for the one-wave-per-ray kernel (another summation order).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import transmittance_bundle_scenes as S
from conftest import ROOT
from transmittance_bundle_scenes import RAY_PL, RAY_LCAP, TOL, SG

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


def oracle_T(oracle, key, o, d, s, g, pair=(1, 1), rays=None):
    """Computed once per (scene, rays, samples, pair) and shared, unchanged, among the tests."""
    return cached(("oracle", key, pair), lambda: S.oracle_T(oracle, o, d, s, g, pair[0], pair[1], rays=rays))


def setup(renderer, g, pair=(1, 1), eps=1e-9):
    renderer.set_gaussians(g)
    renderer.set_options(pair[0], pair[1], eps)
    renderer.clear_tiles()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. parity ----
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("name", ["coherent", "scattered"])
def test_parity_grid16(renderer, oracle, name, pair):
    ex = PAIRS[pair]
    g = grid(oracle, 16)
    o, d = bundle(oracle, name)
    assert (o.size == 3) == (name == "coherent") and len(d) == (130 if name == "coherent" else 32)
    ref = oracle_T(oracle, name, o, d, S.PROFILE_S, g, ex)
    assert (ref[:, -1] < 0.95).any()                           # not a check over empty space
    renderer.enable_stats(True)
    try:
        for eps in (1e-9, 0.0):
            setup(renderer, g, ex, eps)
            T = renderer.transmittance_bundle(o, d, S.PROFILE_S)
            st = renderer.ray_stats()
            lo, hi = S.kept_range(o, d, g, eps, ex[0])
            err = np.abs(T.astype(np.float64) - ref).max(1)
            tol = S.tolerance(lo, hi, len(g), eps)
            print(f"{name} {pair} eps {eps:g}: max err short {err[hi <= RAY_PL].max():.3e} (tol {tol.min():.3e}), "
                  f"other {err[hi > RAY_PL].max() if (hi > RAY_PL).any() else 0:.3e}, lists {lo.min()}..{hi.max()}, stats {st}")
            assert T.shape == (len(d), len(S.PROFILE_S))
            assert st["rays"] == len(d) and st["short_rays"] + st["long_rays"] == len(d)
            assert (lo > RAY_PL).sum() <= st["long_rays"] <= (hi > RAY_PL).sum()
            assert (lo <= RAY_PL).sum() >= st["short_rays"] >= (hi <= RAY_PL).sum()
            assert (err <= tol).all(), (err.max(), (err / tol).max())
            if eps == 0.0:                                      # the full sum on the device, sample by sample
                oo = np.broadcast_to(o.reshape(-1, 3), d.shape)
                full = np.stack([renderer.transmittance_rays(oo, d, np.full(len(d), sv, np.float32)) for sv in S.PROFILE_S], 1)
                short = hi <= RAY_PL
                assert short.any() and np.abs(T[short].astype(np.float64) - full[short]).max() <= 2e-6
                print(f"{name} {pair}: {(bits(T[short]) != bits(full[short])).sum()} of {T[short].size} short-ray values not bit-equal to the full sum")
    finally:
        renderer.enable_stats(False)


# ---- 2. RAY_PL ----
@pytest.mark.parametrize("k, long_rays", [(RAY_PL - 1, 0), (RAY_PL, 0), (RAY_PL + 1, 2)])
def test_list_capacity(renderer, oracle, k, long_rays):
    g = S.stack(oracle, k)
    o, d = S.stack_rays()
    ref = oracle_T(oracle, ("stack", k), o, d, S.STACK_S, g, rays=[0, 1])
    setup(renderer, g)
    renderer.enable_stats(True)
    try:
        T = renderer.transmittance_bundle(o, d, S.STACK_S)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    assert st["long_rays"] == long_rays and st["short_rays"] == 64 - long_rays
    tol = S.TOL_FULL_SUM + S.cull_bound(k) if k <= RAY_PL else TOL
    err = np.abs(T[:2].astype(np.float64) - ref).max()
    print(f"stack {k}: max err {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert (T[2:] == 1.0).all()                                # the rays that miss: Exp(0), exactly


# ---- 3. a lane over the limit does not move its wave-mates ----
def test_one_lane_over_the_limit_does_not_move_its_wave_mates(renderer, oracle):
    at, over = S.one_over_pair(oracle)
    o, d = S.stack_rays()
    res = []
    renderer.enable_stats(True)
    try:
        for g, n_long in ((at, 0), (over, 2)):
            setup(renderer, g)
            res.append(renderer.transmittance_bundle(o, d, S.STACK_S))
            assert renderer.ray_stats()["long_rays"] == n_long
    finally:
        renderer.enable_stats(False)
    np.testing.assert_array_equal(bits(res[0][2:]), bits(res[1][2:]))
    assert res[0][2:].min() < 0.9                              # the wave-mates read the side column, not empty space
    ref = oracle_T(oracle, "one-over", o, d, S.STACK_S, over, rays=[0, 1, 2, 3, 63])
    assert np.abs(res[1][[0, 1, 2, 3, 63]].astype(np.float64) - ref).max() <= TOL
    assert np.abs(res[1][:2] - res[0][:2]).max() >= 10 * TOL   # the extra Gaussian is seen by the axial rays


# ---- 4. RAY_LCAP ----
@pytest.mark.parametrize("n, scratch_rays", [(RAY_LCAP - 1, 0), (RAY_LCAP, 0), (RAY_LCAP + 1, 1)])
def test_lds_capacity_of_the_long_kernel(renderer, oracle, n, scratch_rays):
    sc = S.wide_stack(oracle, RAY_LCAP, n)
    o, d = S.wide_rays()
    ref = oracle_T(oracle, ("wide", n), o, d, S.WIDE_S, sc.g)
    setup(renderer, sc.g)
    T = renderer.transmittance_bundle(o, d, S.WIDE_S)
    err = np.abs(T.astype(np.float64) - ref).max()
    print(f"wide stack {n}: max err {err:.3e}")
    assert err <= TOL
    renderer.enable_stats(True)
    try:
        one = renderer.transmittance_bundle(o, d[:1], S.WIDE_S)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    assert st["long_rays"] == 1 and st["scratch_rays"] == scratch_rays
    np.testing.assert_array_equal(bits(one[0]), bits(T[0]))


# ---- 5. the sample loop ----
@pytest.mark.parametrize("per_ray", [False, True])
def test_sample_loop(renderer, oracle, per_ray):
    """Short and long rays in one wave; every T[r, k] is what an ns = 1 call with that single sample returns, bit for bit."""
    g = S.stack_with_side(oracle, RAY_PL + 1)
    o, d = S.stack_rays()
    setup(renderer, g)
    rng = np.random.default_rng(17)
    nmax = 2 * SG + 1
    s_all = (rng.uniform(3.0, 7.0, size=(len(d), nmax)) if per_ray else np.tile(np.linspace(3.5, 6.5, nmax), (len(d), 1))).astype(np.float32)
    single = np.stack([renderer.transmittance_bundle(o, d, np.ascontiguousarray(s_all[:, k:k + 1]) if per_ray else s_all[0, k:k + 1],
                                                     s_per_ray=per_ray)[:, 0] for k in range(nmax)], 1)
    assert single[:2].min() < 0.5 and single[2:].min() < 0.9 and (single[2:] == 1.0).any()     # long rays, lit wave-mates, free wave-mates
    for ns in (1, SG - 1, SG, SG + 1, 2 * SG + 1):
        s = np.ascontiguousarray(s_all[:, :ns]) if per_ray else s_all[0, :ns]
        T = renderer.transmittance_bundle(o, d, s, s_per_ray=per_ray)
        assert T.shape == (len(d), ns)
        np.testing.assert_array_equal(bits(T), bits(single[:, :ns]), err_msg=f"ns = {ns}")


# ---- 6. bundle and scene sizes ----
@pytest.mark.parametrize("nrays", [1, 63, 64, 65, 130])
def test_bundle_sizes(renderer, oracle, nrays):
    g = grid(oracle, 16)
    o, d = bundle(oracle, "coherent")
    setup(renderer, g)
    T = renderer.transmittance_bundle(o, d[:nrays], S.PROFILE_S)
    ref = oracle_T(oracle, "coherent", o, d, S.PROFILE_S, g)
    lo, hi = S.kept_range(o, d, g)
    assert T.shape == (nrays, len(S.PROFILE_S))
    assert (np.abs(T.astype(np.float64) - ref[:nrays]).max(1) <= S.tolerance(lo, hi, len(g))[:nrays]).all()
    whole = cached("coherent gpu", lambda: renderer.transmittance_bundle(o, d, S.PROFILE_S))
    np.testing.assert_array_equal(bits(T), bits(whole[:nrays]))


@pytest.mark.parametrize("n", [0, 63, 64, 65, 129])
def test_scene_sizes(renderer, oracle, pkg, n):
    g = grid(oracle, 16)[64:64 + n]                                 # rows of the grid that the coherent rays cross
    o, d = bundle(oracle, "coherent")
    for pair in ((1, 1), (0, 0)):
        setup(renderer, g, pair)
        T = renderer.transmittance_bundle(o, d, S.PROFILE_S)
        if n == 0:
            assert (T == renderer.eval_exp(pair[0], np.zeros(1, np.float32))[0]).all() and (T == 1.0).all()     # Exp(0) of the selected kind
    setup(renderer, g)
    if n:
        T = renderer.transmittance_bundle(o, d, S.PROFILE_S)
        ref = oracle_T(oracle, ("rows", n), o, d, S.PROFILE_S, g)
        lo, hi = S.kept_range(o, d, g)
        assert ref.min() < 0.99 and (np.abs(T.astype(np.float64) - ref).max(1) <= S.tolerance(lo, hi, n)).all()


def test_a_permuted_bundle_gives_the_permuted_result(renderer, oracle):
    g = grid(oracle, 16)
    setup(renderer, g)
    o, d = bundle(oracle, "scattered")
    T = renderer.transmittance_bundle(o, d, S.PROFILE_S)
    perm = np.random.default_rng(1).permutation(len(d))
    np.testing.assert_array_equal(bits(renderer.transmittance_bundle(o[perm], d[perm], S.PROFILE_S)), bits(T[perm]))
    s2 = np.random.default_rng(2).uniform(0.0, 8.0, size=(len(d), 5)).astype(np.float32)
    T2 = renderer.transmittance_bundle(o, d, s2)
    np.testing.assert_array_equal(bits(renderer.transmittance_bundle(o[perm], d[perm], np.ascontiguousarray(s2[perm]))), bits(T2[perm]))
    oc, dc = bundle(oracle, "coherent")
    one = renderer.transmittance_bundle(oc, dc, S.PROFILE_S)
    np.testing.assert_array_equal(bits(renderer.transmittance_bundle(np.tile(oc, (len(dc), 1)), dc, S.PROFILE_S)), bits(one))  # one origin == that origin per ray
    np.testing.assert_array_equal(bits(renderer.transmittance_bundle(oc, dc, np.tile(S.PROFILE_S, (len(dc), 1)))), bits(one))  # shared samples == those per ray


# ---- 7. index on = off ----
def index_cases(oracle):
    g16 = grid(oracle, 16)
    return [("grid16 scattered", g16) + bundle(oracle, "scattered") + (S.PROFILE_S,),
            ("stack 32", S.stack(oracle, RAY_PL)) + S.stack_rays() + (S.STACK_S,),
            ("stack 33", S.stack(oracle, RAY_PL + 1)) + S.stack_rays() + (S.STACK_S,),
            ("wide 1025", S.wide_stack(oracle, RAY_LCAP, RAY_LCAP + 1).g) + S.wide_rays() + (S.WIDE_S,)]


def test_index_on_equals_index_off(renderer, oracle):
    try:
        for name, g, o, d, s in index_cases(oracle):
            setup(renderer, g)
            renderer.set_ray_index(0)
            off = renderer.transmittance_bundle(o, d, s)
            renderer.set_ray_index(1)
            on = renderer.transmittance_bundle(o, d, s)
            assert off.min() < 0.9, name
            np.testing.assert_array_equal(bits(on), bits(off), err_msg=name)
    finally:
        renderer.set_ray_index(0)


# ---- 8. the same cull as radiance ----
@pytest.mark.parametrize("index", [0, 1])
def test_same_cull_as_radiance(renderer, oracle, index):
    renderer.enable_stats(True)
    try:
        for name, g, o, d, s in index_cases(oracle):
            setup(renderer, g)
            renderer.set_ray_index(index)
            renderer.radiance_rays(o, d)
            want, want_index = renderer.ray_stats(), renderer.ray_index_stats()
            renderer.transmittance_bundle(o, d, s)
            got, got_index = renderer.ray_stats(), renderer.ray_index_stats()
            assert want["rays"] == len(d) and got == want, name
            assert got_index == want_index and got_index["indexed"] == index, name
    finally:
        renderer.set_ray_index(0)
        renderer.enable_stats(False)


# ---- 9. device form ----
def test_device_form_on_a_callers_stream(renderer, oracle):
    import torch
    g = grid(oracle, 16)
    setup(renderer, g)
    o, d = bundle(oracle, "scattered")
    want = renderer.transmittance_bundle(o, d, S.PROFILE_S)
    s2 = np.random.default_rng(2).uniform(0.0, 8.0, size=(len(d), 5)).astype(np.float32)
    want2 = renderer.transmittance_bundle(o, d, s2)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t_o, t_d, t_s, t_s2 = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o, d, S.PROFILE_S, s2))
        t_T = torch.full(want.shape, -1.0, dtype=torch.float32, device="cuda")
        t_T2 = torch.full(want2.shape, -1.0, dtype=torch.float32, device="cuda")
        st.synchronize()
        renderer.transmittance_bundle_device(len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_s.data_ptr(), len(S.PROFILE_S), 0, t_T.data_ptr(), stream=st.cuda_stream)
        renderer.transmittance_bundle_device(len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_s2.data_ptr(), s2.shape[1], 1, t_T2.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
    np.testing.assert_array_equal(bits(t_T.cpu().numpy()), bits(want))
    np.testing.assert_array_equal(bits(t_T2.cpu().numpy()), bits(want2))


def test_scene_change_right_behind_a_bundle_in_flight(renderer, oracle):
    import torch
    g1, g2 = grid(oracle, 32), S.stack(oracle, RAY_PL + 1)
    o, d = bundle(oracle, "scattered", 32)
    o2, d2 = S.stack_rays()
    o2 = np.tile(o2, (len(d2), 1))
    setup(renderer, g2)
    want2 = renderer.transmittance_bundle(o2, d2, S.STACK_S)
    setup(renderer, g1)
    want1 = renderer.transmittance_bundle(o, d, S.PROFILE_S)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o, d, o2, d2, S.PROFILE_S, S.STACK_S)]
        out1 = torch.zeros(want1.shape, dtype=torch.float32, device="cuda")
        out2 = torch.zeros(want2.shape, dtype=torch.float32, device="cuda")
        again = torch.zeros(want2.shape, dtype=torch.float32, device="cuda")
        st.synchronize()
        renderer.transmittance_bundle_device(len(d), t[0].data_ptr(), 1, t[1].data_ptr(), t[4].data_ptr(), len(S.PROFILE_S), 0, out1.data_ptr(), stream=st.cuda_stream)
        renderer.set_gaussians(g2)                                   # no synchronisation by the caller
        renderer.transmittance_bundle_device(len(d2), t[2].data_ptr(), 1, t[3].data_ptr(), t[5].data_ptr(), len(S.STACK_S), 0, out2.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        renderer.transmittance_bundle_device(len(d2), t[2].data_ptr(), 1, t[3].data_ptr(), t[5].data_ptr(), len(S.STACK_S), 0, again.data_ptr(), stream=st.cuda_stream)
        free_after = torch.cuda.mem_get_info()[0]                    # the second call of the same size: no allocation
        st.synchronize()
    assert want1.min() < 0.9 and want2.min() < 0.9
    np.testing.assert_array_equal(bits(out1.cpu().numpy()), bits(want1))
    np.testing.assert_array_equal(bits(out2.cpu().numpy()), bits(want2))
    np.testing.assert_array_equal(bits(again.cpu().numpy()), bits(want2))
    assert free_after == free_before


# ---- 10. argument errors ----
def test_argument_errors(renderer, oracle, pkg):
    import torch
    setup(renderer, grid(oracle, 16))
    o, d = bundle(oracle, "scattered")
    s = S.PROFILE_S
    L, f32p = pkg.lib(), C.POINTER(C.c_float)
    T = np.full((len(d), len(s)), -1.0, np.float32)
    op, dp, sp, Tp = o.ctypes.data_as(f32p), d.ctypes.data_as(f32p), s.ctypes.data_as(f32p), T.ctypes.data_as(f32p)
    host = L.vrt_hip_transmittance_bundle
    assert host(renderer._h, len(d), op, 1, None, sp, len(s), 0, Tp) == -1      # VRT_HIP_ERR_INVALID
    assert host(renderer._h, len(d), None, 1, dp, sp, len(s), 0, Tp) == -1
    assert host(renderer._h, len(d), op, 1, dp, None, len(s), 0, Tp) == -1
    assert host(renderer._h, len(d), op, 1, dp, sp, len(s), 0, None) == -1
    assert host(None, len(d), op, 1, dp, sp, len(s), 0, Tp) == -1
    assert host(renderer._h, 2 ** 32, op, 1, dp, sp, len(s), 0, Tp) == -1         # more rays than the u32 queue holds
    assert (T == -1.0).all()
    assert host(renderer._h, 0, None, 1, None, None, len(s), 0, None) == 0         # nothing to do
    assert host(renderer._h, len(d), None, 1, None, None, 0, 0, None) == 0
    t_o, t_d, t_s = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o, d, s))
    t_T = torch.full(T.shape, -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev = L.vrt_hip_transmittance_bundle_device
    assert dev(renderer._h, len(d), t_o.data_ptr(), 1, None, t_s.data_ptr(), len(s), 0, t_T.data_ptr(), None) == -1
    assert dev(renderer._h, len(d), None, 1, t_d.data_ptr(), t_s.data_ptr(), len(s), 0, t_T.data_ptr(), None) == -1
    assert dev(renderer._h, len(d), t_o.data_ptr(), 1, t_d.data_ptr(), None, len(s), 0, t_T.data_ptr(), None) == -1
    assert dev(renderer._h, len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_s.data_ptr(), len(s), 0, None, None) == -1
    assert dev(renderer._h, 2 ** 32, t_o.data_ptr(), 1, t_d.data_ptr(), t_s.data_ptr(), len(s), 0, t_T.data_ptr(), None) == -1
    assert dev(renderer._h, 0, None, 1, None, None, len(s), 0, None, None) == 0
    assert dev(renderer._h, len(d), None, 1, None, None, 0, 0, None, None) == 0
    renderer.sync()
    torch.cuda.synchronize()
    assert (t_T.cpu().numpy() == -1.0).all()                         # nothing was enqueued
    with pytest.raises(pkg.VrtHipError):
        renderer.transmittance_bundle_device(len(d), t_o.data_ptr(), 1, t_d.data_ptr(), t_s.data_ptr(), len(s), 0, 0)
    assert renderer.transmittance_bundle(np.zeros(3, np.float32), np.zeros((0, 3), np.float32), s).shape == (0, len(s))


# ---- 11. the C++ example ----
def test_cpp_shadow_rays_example(renderer, oracle):
    """host/shadow_rays_example.cpp (vrt::radiance_rays, then vrt::transmittance_bundle at 8 depths of the same rays): the T and the
    radiance it prints are those of the same rays through the Python binding."""
    p = subprocess.run([os.path.join(BIN, "shadow_rays_example")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    num = r"[-+0-9.e]+|inf|nan"
    rows = [re.fullmatch(rf"ray (\d+) o ((?:(?:{num}) ){{3}})n ((?:(?:{num}) ){{3}})L ((?:(?:{num}) ){{4}})T((?: (?:{num})){{8}})", ln) for ln in p.stdout.strip().splitlines()]
    assert len(rows) == 12 and all(rows), p.stdout
    assert [int(m.group(1)) for m in rows] == list(range(12))
    o, d, L, T = (np.array([[float(v) for v in m.group(k).split()] for m in rows], np.float32) for k in (2, 3, 4, 5))
    g = oracle.gaussians([[0, 1, 0, .1], [0, 0, 1, .7], [1, 0, 0, 1]], [[.3, .3, .5], [-.3, -.3, 0], [0, 0, 2]], [0.1, 0.4, 0.75], [2, .7, 1])
    setup(renderer, g)
    s = (0.5 + np.arange(8)).astype(np.float32)
    np.testing.assert_array_equal(bits(renderer.transmittance_bundle(o, d, s)), bits(T))
    np.testing.assert_array_equal(bits(renderer.radiance_rays(o, d)), bits(L))
    assert T.min() < 0.6 and T.max() > 0.99 and (np.diff(T, axis=1) <= 1e-6).all()          # depth profiles: T falls along a ray
