"""The point queries on the GPU (csrc/vrt_query_kernel.hip behind csrc/vrt_hip_query.cpp): transmittance, transmittance_rays,
transmittance_step, density, radiance -- "the full sums" the bundle suites lean on -- and the Exp / Erf evaluators.  Scenes, float64
models, derived bounds and pair tolerances: tests/query_scenes.py; tests/test_query_scenes.py shows on the CPU that the oracle meets
them and that they see ten wrong kernels.

Against the oracle under the same (Exp, Erf) pair: 2e-6 on T and TOL_NOCULL = 2e-5 on radiance, the constants test_gpu_parity.py applies
to these calls, plus what query_scenes.T_tolerance / radiance_tolerance derive for the samples a pair's format makes sensitive (an Erf or
spline_exp jump within float noise, fast_exp's quantum).  Against the float64 models: inside their bounds.
Every test leaves set_options(EXP_VCL, ERF_AS, 1e-9), no tiles and no shard behind.
"""
import ctypes as C
import os

import numpy as np
import pytest

import query_scenes as Q
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture
def r(pkg, renderer):
    yield renderer
    renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    renderer.clear_tiles()
    renderer.set_shard(0, 1)


def oracle_T(oracle, name, pair):
    """[NRAYS, ns]: computed once per (scene, pair), shared and left unchanged"""
    sc = Q.named_scene(name)
    return cached(("T", name, pair), lambda: np.stack([oracle.transmittance(sc.origins[k], sc.dirs[k], sc.s[k], sc.g, *pair) for k in range(Q.NRAYS)]))


def oracle_L(oracle, name, pair):
    sc = Q.named_scene(name)
    return cached(("L", name, pair), lambda: np.stack([oracle.radiance(sc.origins[k], sc.dirs[k], sc.g, *pair) for k in Q.model_rays(sc)]))


def gpu_T(r, sc):
    return np.stack([r.transmittance(sc.origins[k], sc.dirs[k], sc.s[k]) for k in range(Q.NRAYS)])


# ---- 1. all nine pairs against the oracle ----
@pytest.mark.parametrize("pair", Q.ALL_PAIRS, ids=lambda p: f"exp{p[0]}-erf{p[1]}")
@pytest.mark.parametrize("name", ["ref3", "n65"])
def test_every_pair_against_the_oracle(r, oracle, name, pair):
    """transmittance, transmittance_rays and radiance under each of the nine pairs VRT_DISPATCH_EXP_ERF instantiates."""
    sc = Q.named_scene(name)
    r.set_gaussians(sc.g)
    r.set_options(pair[0], pair[1], 1e-9)
    To, Lo = oracle_T(oracle, name, pair), oracle_L(oracle, name, pair)
    tol_T = np.stack([Q.T_tolerance(sc.origins[k], sc.dirs[k], sc.s[k], sc.g, pair) for k in range(Q.NRAYS)])
    tol_L = np.stack([Q.radiance_tolerance(sc.origins[k], sc.dirs[k], sc.g, pair) for k in range(Q.NRAYS)])
    T = gpu_T(r, sc)
    print(f"{name} {pair}: T off by {np.abs(T - To).max():.3e} (largest tolerance {tol_T.max():.3e}, share {(np.abs(T - To) / tol_T).max():.3f})")
    assert (np.abs(T - To) <= tol_T).all()
    if pair in Q.ACCURATE_PAIRS:
        assert (tol_T == Q.TOL_T).all() and (tol_L == Q.TOL_RADIANCE).all()
    # one sample per ray through transmittance_rays: column 4 of the samples
    Tr = r.transmittance_rays(sc.origins, sc.dirs, sc.s[:, 4])
    assert (np.abs(Tr - To[:, 4]) <= tol_T[:, 4]).all()
    L = r.radiance(sc.origins, sc.dirs)
    print(f"{name} {pair}: radiance off by {np.abs(L - Lo).max():.3e} (largest tolerance {tol_L.max():.3e}, share {(np.abs(L - Lo) / tol_L).max():.3f})")
    assert (np.abs(L - Lo) <= tol_L).all()
    assert np.abs(Lo).max() > 0.05 and To.min() < 0.9


# ---- 2. the accurate pairs against the float64 models, every scene size ----
@pytest.mark.parametrize("name", Q.SCENE_NAMES)
def test_accurate_pairs_inside_the_float64_models(r, oracle, name):
    """n = 0, 1 .. 9 (every residue of the emitter chunk of 4, one and two chunks), 63 / 64 / 65, 1000, the reference's three: T, density and
    radiance inside the models' derived bounds; for n = 1000 the oracle (two rays) inside the same bound around the GPU's radiance."""
    sc = Q.named_scene(name)
    r.set_gaussians(sc.g)
    used = dict(T=0.0, L=0.0, D=0.0)
    for pair in Q.ACCURATE_PAIRS:
        M = cached(("model", name, pair[1]), lambda: Q.models(name, pair[1]))
        r.set_options(pair[0], pair[1], 1e-9)
        T, L = gpu_T(r, sc), r.radiance(sc.origins, sc.dirs)
        rays = list(Q.model_rays(sc))
        assert (np.abs(T - M["T"]) <= M["dT"]).all(), pair
        assert (np.abs(L[rays] - M["L"]) <= M["dL"]).all(), pair
        if sc.n:
            used["T"] = max(used["T"], (np.abs(T - M["T"]) / M["dT"]).max())
            used["L"] = max(used["L"], (np.abs(L[rays] - M["L"]) / M["dL"]).max())
        if pair in ((0, 0), (1, 1)):
            To, Lo = oracle_T(oracle, name, pair), oracle_L(oracle, name, pair)
            tol_T = Q.TOL_T if sc.n <= 65 else np.maximum(Q.TOL_T, M["dT"])
            tol_L = Q.TOL_RADIANCE if sc.n <= 65 else np.maximum(Q.TOL_RADIANCE, M["dL"])
            print(f"{name} {pair}: T - oracle {np.abs(T - To).max():.3e}, radiance - oracle {np.abs(L[rays] - Lo).max():.3e}")
            assert (np.abs(T - To) <= tol_T).all() and (np.abs(L[rays] - Lo) <= tol_L).all(), pair
    D = r.density(sc.pts)
    M = Q.models(name, 0)
    assert (np.abs(D - M["D"]) <= M["dD"]).all()
    if sc.n:
        used["D"] = (np.abs(D - M["D"]) / M["dD"]).max()
        Do = np.array([oracle.density(p, sc.g) for p in sc.pts], np.float32)
        assert np.abs(D - Do).max() <= max(1e-6, M["dD"].max())       # test_gpu_parity.py's constant for density
    print(f"{name}: share of the models' bounds used {used}")


def test_empty_scene_overwrites_garbage(r, pkg):
    """n = 0: T = 1, density 0, radiance 0 -- written, not left over: the output arrays hold garbage beforehand."""
    sc = Q.named_scene("n5")
    r.set_gaussians(sc.g[:0])
    L, f32p = pkg.lib(), C.POINTER(C.c_float)
    p = lambda a: a.ctypes.data_as(f32p)
    o, d, s = np.ascontiguousarray(sc.origins), np.ascontiguousarray(sc.dirs), np.ascontiguousarray(sc.s[0])
    for ek, rk in Q.ALL_PAIRS:
        r.set_options(ek, rk, 1e-9)
        T = np.full(len(s), np.nan, np.float32)
        assert L.vrt_hip_transmittance(r._h, p(o[0]), p(d[0]), p(s), len(s), p(T)) == 0
        # Exp(0) of the pair: 1 but for fast_exp (0.97816086, approx.cpp:112-129)
        assert (T == (np.float32(0.97816086) if ek == 2 else 1)).all(), (ek, rk, T)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    T = np.full(Q.NRAYS, np.nan, np.float32)
    assert L.vrt_hip_transmittance_rays(r._h, Q.NRAYS, p(o), p(d), p(np.ascontiguousarray(sc.s[:, 3])), p(T)) == 0 and (T == 1).all()
    D = np.full(len(sc.pts), np.nan, np.float32)
    assert L.vrt_hip_density(r._h, len(sc.pts), p(np.ascontiguousarray(sc.pts)), p(D)) == 0 and (D == 0).all()
    out = np.full((Q.NRAYS, 4), np.nan, np.float32)
    assert L.vrt_hip_radiance(r._h, Q.NRAYS, p(o), p(d), p(out)) == 0 and (out == 0).all()
    Ts = np.full(len(s), np.nan, np.float32)
    assert L.vrt_hip_transmittance_step(r._h, p(o[0]), p(d[0]), p(s), len(s), C.c_float(0.25), p(Ts)) == 0
    assert (Ts == np.float32(0.97816086)).all()


# ---- 3. launch shapes ----
def many_rays(sc, n, seed=5):
    """n rays around the scene's own: its eight first, then jittered copies"""
    rng = np.random.default_rng(seed)
    k = np.arange(n) % Q.NRAYS
    o = sc.origins[k] + (rng.normal(size=(n, 3)) * 0.05 * (np.arange(n) >= Q.NRAYS)[:, None]).astype(np.float32)
    d = Q.unit(sc.dirs[k].astype(np.float64) + rng.normal(size=(n, 3)) * 0.03 * (np.arange(n) >= Q.NRAYS)[:, None])
    s = rng.uniform(-1.0, 8.0, n).astype(np.float32)
    return np.ascontiguousarray(o.astype(np.float32)), d, s


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_launch_shapes(r, oracle, n):
    """ns, nrays, npts either side of the wave of 64: every result the one the same input gives in a launch of 130, and the oracle's at a sample of them."""
    sc = Q.named_scene("n9")
    r.set_gaussians(sc.g)
    o, d, s = many_rays(sc, 130)
    full = cached("shapes", lambda: dict(T=r.transmittance(o[0], d[0], s), Tr=r.transmittance_rays(o, d, s), L=r.radiance(o, d), D=r.density(o + d * s[:, None]),
                                         Ts=r.transmittance_step(o[0], d[0], s, 0.25)))
    T, Tr, L, D = r.transmittance(o[0], d[0], s[:n]), r.transmittance_rays(o[:n], d[:n], s[:n]), r.radiance(o[:n], d[:n]), r.density((o + d * s[:, None])[:n])
    Ts = r.transmittance_step(o[0], d[0], s[:n], 0.25)
    assert T.shape == Tr.shape == D.shape == Ts.shape == (n,) and L.shape == (n, 4)
    for got, ref in ((T, full["T"]), (Tr, full["Tr"]), (L, full["L"]), (D, full["D"]), (Ts, full["Ts"])):
        np.testing.assert_array_equal(bits(got), bits(ref[:n]))
    for k in sorted({0, n // 2, n - 1} & set(range(n))):
        assert abs(Tr[k] - oracle.transmittance(o[k], d[k], s[k:k + 1], sc.g, 1, 1)[0]) <= Q.TOL_T
        assert np.abs(L[k] - oracle.radiance(o[k], d[k], sc.g, 1, 1)).max() <= Q.TOL_RADIANCE
        assert abs(T[k] - oracle.transmittance(o[0], d[0], s[k:k + 1], sc.g, 1, 1)[0]) <= Q.TOL_T
        assert abs(D[k] - oracle.density(o[k] + d[k] * s[k], sc.g)) <= 1e-6


@pytest.mark.parametrize("n", [0, 255, 256, 257])
def test_evaluator_launch_shapes(r, pkg, oracle, n):
    """vrt_hip_eval_erf / _exp, blocks of 256: every kind at n either side of a block, against the oracle's functions"""
    x = np.linspace(-4.0, 4.0, n).astype(np.float32)
    for kind, fn, tol in ((pkg.ERF_AS, "oracle_as_erf", 5e-7), (pkg.ERF_SPLINE, "oracle_spline_erf", 5e-7), (pkg.ERF_SPLINE_MIRROR, "oracle_spline_erf_mirror", 5e-7),
                          (pkg.ERF_TAYLOR, "oracle_taylor_erf", 2e-6)):
        y = r.eval_erf(kind, x)
        assert y.shape == (n,) and (n == 0 or np.abs(y - oracle.map_scalar(fn, x)).max() <= tol), fn
    for kind, fn in ((pkg.EXP_VCL, "oracle_vcl_exp"), (pkg.EXP_FAST, "oracle_fast_exp"), (pkg.EXP_SPLINE, "oracle_spline_exp")):
        y, ref = r.eval_exp(kind, -x - 4), oracle.map_scalar(fn, -x - 4)
        assert y.shape == (n,) and (np.abs(y - ref) <= 2.5e-7 * np.abs(ref)).all(), fn


@pytest.mark.parametrize("nrays", [65, 130])
def test_a_ray_gives_the_same_bits_wherever_it_travels(r, nrays):
    """One ray at index 0, in the middle of a wave and last -- the last wave has lanes past nrays, which read the clamped index rc -- and
    alone: the same bits.  Under a pair of each emission_term form."""
    sc = Q.named_scene("n65")
    r.set_gaussians(sc.g)
    o, d, s = many_rays(sc, nrays, seed=9)
    for pair in ((1, 1), (2, 1), (1, 3)):
        r.set_options(pair[0], pair[1], 1e-9)
        alone_L, alone_T = r.radiance(sc.origins[3:4], sc.dirs[3:4]), r.transmittance_rays(sc.origins[3:4], sc.dirs[3:4], sc.s[3, 5:6])
        for at in (0, 37, 64, nrays - 1):
            oo, dd, ss = o.copy(), d.copy(), s.copy()
            oo[at], dd[at], ss[at] = sc.origins[3], sc.dirs[3], sc.s[3, 5]
            L, T = r.radiance(oo, dd), r.transmittance_rays(oo, dd, ss)
            np.testing.assert_array_equal(bits(L[at]), bits(alone_L[0]), err_msg=f"{pair} radiance at {at} of {nrays}")
            assert bits(T[at:at + 1])[0] == bits(alone_T)[0], (pair, at, nrays)
            others = np.arange(nrays) != at
            if at == 0:
                base_L, base_T = L, T
            else:       # and the rays that travel with it do not depend on it
                keep = others & (np.arange(nrays) != 0)
                np.testing.assert_array_equal(bits(L[keep]), bits(base_L[keep]))
                np.testing.assert_array_equal(bits(T[keep]), bits(base_T[keep]))


# ---- 4. identities, bit for bit ----
def frame_setup(r, oracle, w=64, tiles_n=4):
    cam, _ = oracle.cli_camera(w, w)
    r.set_plane(w, w, *oracle.camera_plane(cam))
    return cam, np.array(cam.position[:], np.float32)


def all_queries(r, sc):
    return [gpu_T(r, sc), r.transmittance_rays(sc.origins, sc.dirs, sc.s[:, 6]), r.radiance(sc.origins, sc.dirs), r.density(sc.pts),
            r.transmittance_step(sc.origins[1], sc.dirs[1], sc.s[1], 0.25)]


def test_rays_entry_point_equals_the_one_ray_entry_point(r):
    sc = Q.named_scene("n65")
    r.set_gaussians(sc.g)
    o, d, s = many_rays(sc, 130)
    for pair in ((1, 1), (0, 0), (3, 1), (1, 4)):
        r.set_options(pair[0], pair[1], 1e-9)
        Tr = r.transmittance_rays(o, d, s)
        for k in range(130):
            assert bits(Tr[k:k + 1])[0] == bits(r.transmittance(o[k], d[k], s[k:k + 1]))[0], (pair, k)


def test_full_sums_read_no_cull_column_table_setting_shard_or_tiles(r, pkg, oracle):
    """cull_eps 0 / 1e-9 / 1e-3, table step 0 / default, a shard and tiles set: the same bits from every query"""
    sc = Q.named_scene("n65")
    r.set_gaussians(sc.g)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    ref = all_queries(r, sc)
    cam, origin = frame_setup(r, oracle)
    for eps, step, shard, tiles in ((0.0, None, None, False), (1e-3, None, None, False), (1e-9, 0.0, None, False), (1e-9, None, (1, 2), True), (1e-3, 0.0, (0, 4), True)):
        r.set_options(pkg.EXP_VCL, pkg.ERF_AS, eps)
        r.set_table_step(pkg.TABLE_STEP_DEFAULT if step is None else step)
        if tiles:
            r.tile_gaussians(2 / 4, 2 / 4, oracle.camera_view(cam))
        else:
            r.clear_tiles()
        r.set_shard(*(shard or (0, 1)))
        for got, want in zip(all_queries(r, sc), ref):
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=str((eps, step, shard, tiles)))
    r.set_table_step(pkg.TABLE_STEP_DEFAULT)


def test_aos_and_soa_uploads_give_the_same_bits(r):
    sc = Q.named_scene("n65")
    r.set_gaussians(sc.g)
    ref = all_queries(r, sc)
    g = sc.g
    r.set_gaussians_soa(g["mu"][:, :3], g["albedo"][:, :3], g["sigma"], g["magnitude"], alpha=g["albedo"][:, 3])
    for got, want in zip(all_queries(r, sc), ref):
        np.testing.assert_array_equal(bits(got), bits(want))


# ---- 5. state ----
def test_a_query_is_the_first_call_after_set_gaussians(pkg, oracle):
    """a fresh context: scene, then a query -- no frame rendered, no options set (the defaults are vcl_exp, A&S erf)"""
    sc = Q.named_scene("n9")
    fresh = pkg.Renderer(0)
    try:
        fresh.set_gaussians(sc.g)
        L = fresh.radiance(sc.origins, sc.dirs)
        assert np.abs(L - oracle_L(oracle, "n9", (1, 1))).max() <= Q.TOL_RADIANCE
        fresh.set_gaussians(sc.g[:3])
        T = fresh.transmittance(sc.origins[0], sc.dirs[0], sc.s[0])
        assert np.abs(T - oracle.transmittance(sc.origins[0], sc.dirs[0], sc.s[0], sc.g[:3], 1, 1)).max() <= Q.TOL_T
    finally:
        fresh.close()


def test_a_scene_grows_shrinks_and_grows(r, oracle):
    """5 -> 1000 -> 0 -> 3 Gaussians in one context: iota and the tables follow"""
    for name, g in (("n5", None), ("n1000", None), ("n0", None), ("three", Q.named_scene("n9").g[:3]), ("n65", None)):
        sc = Q.named_scene("n9" if g is not None else name)
        g = sc.g if g is None else g
        r.set_gaussians(g)
        rays = range(2)
        L, T, D = r.radiance(sc.origins, sc.dirs), gpu_T(r, sc), r.density(sc.pts)
        if name == "three":
            Lo = np.stack([oracle.radiance(sc.origins[k], sc.dirs[k], g, 1, 1) for k in rays])
            To = np.stack([oracle.transmittance(sc.origins[k], sc.dirs[k], sc.s[k], g, 1, 1) for k in rays])
        else:
            Lo, To = oracle_L(oracle, name, (1, 1))[:2], oracle_T(oracle, name, (1, 1))[:2]
        M = Q.models(name, 1) if name == "n1000" else None
        assert (np.abs(L[:2] - Lo) <= (Q.TOL_RADIANCE if M is None else np.maximum(Q.TOL_RADIANCE, M["dL"]))).all(), name
        assert (np.abs(T[:2] - To) <= (Q.TOL_T if M is None else np.maximum(Q.TOL_T, M["dT"][:2]))).all(), name
        assert np.abs(D - np.array([oracle.density(p, g) for p in sc.pts], np.float32)).max() <= 1e-6, name


def test_a_query_between_two_frames_leaves_them_alone(r, pkg, oracle):
    """frame, query, frame with a moved camera: both frames bit-equal to the same frames rendered without the query, the query's result
    the one it gives on its own"""
    sc = Q.named_scene("n65")
    r.set_gaussians(sc.g)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    alone = all_queries(r, sc)
    w = 64
    cams = [oracle.cli_camera(w, w, initial_rot=rot)[0] for rot in (0.0, 25.0)]

    def frame(cam):
        r.set_plane(w, w, *oracle.camera_plane(cam))
        r.tile_gaussians(2 / 4, 2 / 4, oracle.camera_view(cam))
        return r.render(np.array(cam.position[:], np.float32))

    plain = [frame(c) for c in cams]
    assert plain[0][1].max() > 0.05
    first = frame(cams[0])
    between = all_queries(r, sc)
    second = frame(cams[1])
    for (img, rad), (img0, rad0) in zip((first, second), plain):
        np.testing.assert_array_equal(img, img0)
        np.testing.assert_array_equal(bits(rad), bits(rad0))
    for got, want in zip(between, alone):
        np.testing.assert_array_equal(bits(got), bits(want))


# ---- 6. the step sum ----
@pytest.mark.parametrize("name", ["ref3", "n5", "n65"])
@pytest.mark.parametrize("delta,reach", Q.STEP_CASES)
def test_step_sum_inside_its_model(r, oracle, name, delta, reach):
    """Against the float32 t sequence summed in float64 (query_scenes.step_model), inside its bound -- which the loop with `<`, one step short
    where a sample lies exactly on a step, misses by far (asserted here on the model, and shown for ten variants on the CPU).  Samples: 0,
    negative and NaN (zero steps: fast_exp(-0)), exactly on a step, one ulp either side, in between; at most 2000 steps over 65 Gaussians."""
    sc = Q.named_scene(name)
    r.set_gaussians(sc.g)
    s = Q.step_samples(delta, reach)
    used = strict = 0.0
    for k in (0, 3):
        T = r.transmittance_step(sc.origins[k], sc.dirs[k], s, delta)
        for v, got in zip(s, T):
            want, bound, steps = Q.step_model(oracle, sc.origins[k], sc.dirs[k], v, delta, sc.g)
            assert steps <= 2000
            assert abs(got - want) <= bound, (name, delta, k, v, got, want, bound)
            used = max(used, abs(got - want) / bound)
            strict = max(strict, abs(Q.step_model(oracle, sc.origins[k], sc.dirs[k], v, delta, sc.g, "step_strict")[0] - want) / bound)
            if not v >= 0:
                assert got == np.float32(0.97816086)
    print(f"{name} delta {delta}: share of the bound used {used:.3f}; the loop with < would be off by {strict:.1f} bounds")
    assert strict >= 10


def test_step_sum_refuses_what_would_not_end(r, pkg):
    """The refusals of csrc/vrt_step_guard.hpp reach the caller as VRT_HIP_ERR_INVALID with the reason, and nothing is launched: only the error
    code and the message are asserted, for the refused rows of the guard's table (the accepted rows are replayed on the CPU)."""
    sc = Q.named_scene("n65")
    r.set_gaussians(sc.g)
    L, f32p = pkg.lib(), C.POINTER(C.c_float)
    words = {1: "delta must be a normal positive float", 2: "+inf", 3: "delta * 2^23", 4: "2^23 density evaluations"}
    refused = 0
    for s_txt, delta_txt, n, refusal in Q.GUARD_TABLE:
        if not refusal or (refusal == 4 and n > sc.n):
            continue        # (a work-cap row is refused for its n: only those this scene's 65 Gaussians refuse as well)
        conv = lambda v: float.fromhex(v) if "x" in v else float(v)
        s = np.array([conv(v) for v in s_txt.split(",")], np.float32)
        delta = np.float32(conv(delta_txt))
        T = np.full(len(s), -2.0, np.float32)
        rc = L.vrt_hip_transmittance_step(r._h, sc.origins[0].ctypes.data_as(f32p), sc.dirs[0].ctypes.data_as(f32p), s.ctypes.data_as(f32p), len(s),
                                          C.c_float(float(delta)), T.ctypes.data_as(f32p))
        assert rc == -1 and (T == -2.0).all(), (s_txt, delta_txt)
        if delta > 0:       # (delta <= 0 and NaN fail the argument check before the guard, without a message of their own)
            assert words[refusal] in L.vrt_hip_last_error(r._h).decode(), (s_txt, delta_txt, L.vrt_hip_last_error(r._h))
        refused += 1
    assert refused >= 12
    for s, delta, word in (([1.0, np.inf], 0.01, "never end"), ([3e5], 0.01, "round back"), ([2.0 ** 21], 1.0, "2\\^23 density"), ([1.0], 1e-40, "normal positive")):
        with pytest.raises(pkg.VrtHipError, match=word):
            r.transmittance_step(sc.origins[0], sc.dirs[0], np.float32(s), delta)
    # and the context is as usable as before
    assert r.transmittance_step(sc.origins[0], sc.dirs[0], np.float32([np.nan, -1.0]), 0.01).tolist() == [np.float32(0.97816086)] * 2


# ---- 7. the evaluators at their edges ----
def test_evaluators_at_their_edges(r, pkg, oracle):
    """tests/golden/approx_edges.npz: the real approx.cpp at +-0, the smallest normal, a subnormal, the splines' piece borders, |x| = 2, +-87.3,
    +-88.7 and either side of fast_exp's clamps, within the constants of test_gpu_parity.py::test_device_erf_exp_against_reference_tables;
    fast_exp bit for bit the oracle's; where the table holds 0 or +inf (vcl_exp from -87.3 down, expf past FLT_MAX, fast_exp's clamps) the device
    holds the same.  vcl_exp from +87.3 up has a test of its own below."""
    e = np.load(os.path.join(GOLDEN, "approx_edges.npz"))
    x, xe = e["erf_x"], e["exp_x"]
    for kind, key, tol in ((pkg.ERF_AS, "as_erf", 5e-7), (pkg.ERF_SPLINE, "spline_erf", 5e-7), (pkg.ERF_SPLINE_MIRROR, "spline_erf_mirror", 5e-7),
                           (pkg.ERF_TAYLOR, "taylor_erf", 2e-6), (pkg.ERF_LIBM, "libm_erf", 5e-7)):
        err = np.abs(r.eval_erf(kind, x) - e[key])
        assert err.max() <= tol, (key, x[err.argmax()], err.max())
    v, gold = r.eval_exp(pkg.EXP_VCL, xe), e["vcl_exp"]
    below = xe < np.float32(87.3)            # (from +87.3 up: test_vcl_exp_beyond_its_upper_limit, with +inf)
    fin = below & (gold != 0)
    assert (np.abs(v[fin] - gold[fin]) <= 2.5e-7 * np.abs(gold[fin])).all(), xe[fin][~(np.abs(v[fin] - gold[fin]) <= 2.5e-7 * np.abs(gold[fin]))]
    np.testing.assert_array_equal(v[below & (gold == 0)], 0)       # 0 from -87.3 down, -87.3 itself included
    assert (gold == 0).sum() >= 4 and np.isfinite(gold[below]).all()
    fe = r.eval_exp(pkg.EXP_FAST, xe)
    np.testing.assert_array_equal(bits(fe), bits(oracle.map_scalar("oracle_fast_exp", xe)))
    fg = e["fast_exp"]
    ends = ~np.isfinite(fg) | (fg == 0)
    np.testing.assert_array_equal(fe[ends], fg[ends])
    assert (np.abs(fe[~ends] - fg[~ends]) <= 1e-5 * np.abs(fg[~ends])).all()
    assert np.abs(r.eval_exp(pkg.EXP_SPLINE, xe) - e["spline_exp"]).max() <= 1e-7
    le, lg = r.eval_exp(pkg.EXP_LIBM, xe), e["libm_exp"]
    ok = np.isfinite(lg) & (lg >= 2.0 ** -126)
    assert (np.abs(le[ok] - lg[ok]) <= 2.5e-7 * np.abs(lg[ok])).all()
    np.testing.assert_array_equal(le[np.isinf(lg)], lg[np.isinf(lg)])       # +inf once exp(x) passes FLT_MAX
    assert np.isinf(lg).sum() >= 4 and (np.abs(le[lg < 2.0 ** -126]) <= 2.0 ** -125).all()     # a subnormal result may be flushed


def test_vcl_exp_beyond_its_upper_limit(r, pkg, oracle):
    """The reference's vcl_exp is +inf from x = +87.3 up (the table's rows 87.3, 87.30001, 88.7 and its neighbours, 88.7531 = fast_exp's upper
    clamp and its neighbours, 88.7431, 88.7631; the oracle agrees and gives +inf at +inf too), and so must the device be.  exp_accurate on its
    own gave exp(x) there while that is a float (8.2018e+37 at 87.3, 3.3260e+38 at 88.7), then +inf or NaN: beyond 88.72 its correction term is
    inf * e + inf, NaN for e <= 0 (88.7431, +inf).  exp_vcl restates the limit inside that last fma (vrt_device_math.h)."""
    e = np.load(os.path.join(GOLDEN, "approx_edges.npz"))
    xe, gold = e["exp_x"], e["vcl_exp"]
    up = xe >= np.float32(87.3)
    assert up.sum() >= 9 and np.isinf(gold[up]).all()
    x = np.concatenate([xe[up], np.float32([np.inf])])
    want = oracle.map_scalar("oracle_vcl_exp", x)
    np.testing.assert_array_equal(want[:-1], gold[up])
    got = r.eval_exp(pkg.EXP_VCL, x)
    print("x", x, "device", got, "reference", want)
    np.testing.assert_array_equal(got, want)


def test_evaluators_at_inf_and_nan(r, pkg, oracle):
    """+-inf and NaN: the reference defines nothing there (a -ffast-math build), so the device is held to the oracle's C functions alone --
    the limits they state (Erf +-1, Exp 0 / inf, fast_exp's clamps) and NaN where they give NaN."""
    x = np.array([np.inf, -np.inf, np.nan], np.float32)
    for kind, fn in ((pkg.ERF_AS, "oracle_as_erf"), (pkg.ERF_SPLINE, "oracle_spline_erf"), (pkg.ERF_SPLINE_MIRROR, "oracle_spline_erf_mirror"),
                     (pkg.ERF_TAYLOR, "oracle_taylor_erf")):
        got, want = r.eval_erf(kind, x), oracle.map_scalar(fn, x)
        np.testing.assert_array_equal(got[:2], want[:2], err_msg=fn)
        assert np.isnan(got[2]) == np.isnan(want[2]) and (np.isnan(want[2]) or got[2] == want[2]), (fn, got, want)
    for kind, fn in ((pkg.EXP_VCL, "oracle_vcl_exp"), (pkg.EXP_FAST, "oracle_fast_exp"), (pkg.EXP_SPLINE, "oracle_spline_exp")):
        got, want = r.eval_exp(kind, x), oracle.map_scalar(fn, x)
        np.testing.assert_array_equal(got[:2], want[:2], err_msg=fn)
        if fn != "oracle_fast_exp":     # (fast_exp casts a x + b to unsigned: of a NaN, C leaves that undefined)
            assert np.isnan(got[2]) == np.isnan(want[2]) and (np.isnan(want[2]) or got[2] == want[2]), (fn, got, want)
    le = r.eval_exp(pkg.EXP_LIBM, x)
    assert le[0] == np.inf and le[1] == 0 and np.isnan(le[2])        # expf's own limits
