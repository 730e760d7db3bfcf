"""CPU checks of the point-query suite (tests/query_scenes.py, run on the GPU by tests/test_gpu_queries.py): the scenes are what they
claim, the oracle lies inside every model bound with no sample left out, the scenes see ten wrong kernels at ten tolerances or more,
and the guard of vrt_hip_transmittance_step (csrc/vrt_step_guard.hpp) refuses exactly the arguments its float32 loop does not survive."""
import os
import subprocess

import numpy as np
import pytest

import query_scenes as Q
from conftest import ROOT


def test_scenes_keep_their_limits_and_markers():
    for name in Q.SCENE_NAMES:
        sc = Q.named_scene(name)
        g = sc.g
        assert sc.origins.dtype == sc.dirs.dtype == sc.s.dtype == sc.pts.dtype == np.float32
        assert np.abs(np.linalg.norm(sc.dirs.astype(np.float64), axis=1) - 1).max() <= 1e-7
        if not sc.n:
            continue
        assert g["sigma"].min() >= np.float32(0.1)
        if name == "ref3":      # the reference's own scene, as it is: its far Gaussian is 7 from the origin
            continue
        assert np.linalg.norm(g["mu"][None, :, :3].astype(np.float64) - sc.origins[:, None, :], axis=2).max() <= 6.0
        if sc.n < 5:
            continue
        G = Q.Geometry(sc.origins[0], sc.dirs[0], g)
        dist = np.sqrt(np.maximum(G.c2 - G.mubar ** 2, 0))
        assert g["magnitude"][0] == 0 and g["magnitude"][1] < 0 and G.mubar[2] < 0
        assert dist[3] <= G.sigma[3] / 10 and np.sqrt(G.c2[4]) < G.sigma[4]
        assert (g["magnitude"][5:] > 0).all()
    assert sorted({Q.scene(n).n % 4 for n in Q.SIZES if 0 < n < 10}) == [0, 1, 2, 3]


@pytest.mark.parametrize("n", [5, 9, 65])
def test_markers(n):
    """Without marker j (for j = 0: with magnitude 1), a value the GPU suite checks on ray 0 -- T at a sample, a channel of the radiance --
    moves by at least ten of the tolerances it is checked with there."""
    sc = Q.scene(n)
    o, d = sc.origins[0], sc.dirs[0]
    for erf_kind in (0, 1):
        T, dT = Q.T_model(o, d, sc.s[0], sc.g, erf_kind)
        L, dL = Q.radiance_model(o, d, sc.g, erf_kind)
        for j, what in Q.MARKERS.items():
            g = sc.g.copy()
            if j == 0:
                g["magnitude"][0] = 1.0
            else:
                g = np.delete(g, j)
            moved = max((np.abs(Q.T_model(o, d, sc.s[0], g, erf_kind)[0] - T) / dT).max(),
                        (np.abs(Q.radiance_model(o, d, g, erf_kind)[0] - L) / dL).max())
            assert moved >= Q.MARKER_FACTOR, (n, what, moved)
    # T > 1 behind the origin: rt.h has no clamp
    assert T[sc.s[0] < 0].min() > 1.0 + 100 * dT.max()


def test_oracle_lies_inside_the_models(oracle):
    """The reference implementation alone meets what the GPU test demands: oracle.transmittance, density and radiance under the four accurate
    pairs inside the float64 models' bounds on every scene, ray, sample and point -- none left out.  Prints how much of the bound is used."""
    worst = dict(T=0.0, L=0.0, D=0.0)
    for name in Q.SCENE_NAMES:
        sc = Q.named_scene(name)
        for ek, rk in Q.ACCURATE_PAIRS:
            M = Q.models(name, rk)
            T = np.stack([oracle.transmittance(sc.origins[r], sc.dirs[r], sc.s[r], sc.g, ek, rk) for r in range(Q.NRAYS)])
            assert (np.abs(T - M["T"]) <= M["dT"]).all(), (name, ek, rk)
            worst["T"] = max(worst["T"], (np.abs(T - M["T"]) / M["dT"]).max())
            if sc.n == 1000 and (ek, rk) not in ((0, 0), (1, 1)):
                continue
            L = np.stack([oracle.radiance(sc.origins[r], sc.dirs[r], sc.g, ek, rk) for r in Q.model_rays(sc)])
            assert (np.abs(L - M["L"]) <= M["dL"]).all(), (name, ek, rk)
            if sc.n:
                worst["L"] = max(worst["L"], (np.abs(L - M["L"]) / M["dL"]).max())
        M = Q.models(name, 0)
        D = np.array([oracle.density(p, sc.g) for p in sc.pts], np.float64)
        assert (np.abs(D - M["D"]) <= M["dD"]).all(), name
        if sc.n:
            worst["D"] = max(worst["D"], (np.abs(D - M["D"]) / M["dD"]).max())
        else:
            assert (T == 1).all() and (L == 0).all() and (D == 0).all()
    print("share of the bound the oracle uses:", worst)
    assert all(v > 1e-3 for v in worst.values())     # the bounds are not so wide that nothing registers


@pytest.mark.parametrize("name", ["ref3", "n5", "n65"])
def test_oracle_step_sum_lies_inside_its_model(oracle, name):
    sc = Q.named_scene(name)
    used = 0.0
    for delta, reach in Q.STEP_CASES:
        for r in (0, 3):
            for s in Q.step_samples(delta, reach):
                T, dT, steps = Q.step_model(oracle, sc.origins[r], sc.dirs[r], s, delta, sc.g)
                assert steps <= 2000 and steps * sc.n <= 2000 * 65
                got = oracle.transmittance_step(sc.origins[r], sc.dirs[r], s, delta, sc.g)
                assert abs(got - T) <= dT, (name, delta, r, s, got, T, dT)
                used = max(used, abs(got - T) / dT)
                if not s >= 0:
                    assert steps == 0 and got == oracle.map_scalar("oracle_fast_exp", np.float32([-0.0]))[0]
    print("share of the bound the oracle uses:", used)


def test_oracle_step_sum_refuses_what_would_spin(oracle):
    sc = Q.named_scene("ref3")
    o, d = sc.origins[0], sc.dirs[0]
    for s, delta in ((np.inf, 0.01), (3e5, 0.01), (83886.08, 0.01), (8192.0, 2.0 ** -10), (1.0, 0.0), (1.0, -1.0), (1.0, 1e-40), (1.0, np.nan)):
        with pytest.raises(ValueError):
            oracle.transmittance_step(o, d, s, delta, sc.g)
        with pytest.raises(AssertionError):
            Q.step_times(s, delta)
    assert oracle.transmittance_step(o, d, np.nan, 0.01, sc.g) == oracle.transmittance_step(o, d, -np.inf, 0.01, sc.g)


def _moved(value, wrong, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(np.asarray(wrong) - np.asarray(value)) / np.asarray(bound)
    return float(np.nanmax(q)) if np.size(q) else 0.0


@pytest.mark.parametrize("variant", sorted(Q.VARIANTS))
def test_the_scenes_see_a_wrong_kernel(oracle, variant):
    """Each wrong kernel moves a value the GPU suite checks, on one of its scenes, by ten or more of the tolerances it is checked with."""
    kind = Q.VARIANTS[variant]
    best = 0.0
    for name in ("n5", "n7", "n9", "n65"):
        sc = Q.named_scene(name)
        for r in (0, 3):
            o, d = sc.origins[r], sc.dirs[r]
            if kind == "step":
                for delta, reach in Q.STEP_CASES:
                    for s in Q.step_samples(delta, reach):
                        T, dT, _ = Q.step_model(oracle, o, d, s, delta, sc.g)
                        best = max(best, abs(Q.step_model(oracle, o, d, s, delta, sc.g, variant)[0] - T) / dT)
            elif kind == "density":
                D, dD = Q.density_model(sc.pts, sc.g)
                best = max(best, _moved(D, Q.density_model(sc.pts, sc.g, variant)[0], dD))
            else:
                for erf_kind in (0, 1):
                    M = Q.models(name, erf_kind)
                    if kind == "T":
                        best = max(best, _moved(M["T"][r], Q.T_model(o, d, sc.s[r], sc.g, erf_kind, variant)[0], M["dT"][r]))
                    best = max(best, _moved(M["L"][r], Q.radiance_model(o, d, sc.g, erf_kind, variant)[0], M["dL"][r]))
    assert best >= 10.0, (variant, best)


def test_jump_tables(oracle):
    """ERF_JUMPS / EXP_JUMPS hold the discontinuities of the oracle's functions: at every listed place the function steps by the listed amount,
    rounded up by at most 2 %; spline_exp's step at 0 sits between -FLT_MIN and the subnormals, which the reference reads as 0."""
    f32 = np.float32
    fns = {2: "oracle_spline_erf", 3: "oracle_spline_erf_mirror", 4: "oracle_taylor_erf"}
    for table, names in ((Q.ERF_JUMPS, fns), (Q.EXP_JUMPS, {3: "oracle_spline_exp"})):
        for kind, jumps in table.items():
            for x0, jump in jumps:
                b = f32(x0)
                lo, hi = (f32(-2.0 ** -126), f32(0.0)) if x0 == 0 else (np.nextafter(b, f32(-np.inf)), np.nextafter(b, f32(np.inf)))
                v = oracle.map_scalar(names[kind], np.array([lo, b, hi], f32)).astype(np.float64)
                step = max(abs(v[1] - v[0]), abs(v[2] - v[1]))
                assert step <= jump <= 1.02 * step + 2e-7, (names[kind], x0, step, jump)


def test_pair_tolerances():
    """The accurate pairs get the project's constants and nothing else; spline_erf_mirror lists every emitter's own sample k = 0 (its argument
    (mubar_i - mubar_i) r_i is 0 but for the rounding of two products), and a sample point at a Gaussian's own mubar for T; taylor_erf one at
    |x| = 2; spline_exp a ray through a centre (x = 0) and the sample s = 0 (E = 0)."""
    sc = Q.named_scene("n65")
    o, d = sc.origins[0], sc.dirs[0]
    for pair in Q.ACCURATE_PAIRS:
        assert (Q.T_tolerance(o, d, sc.s[0], sc.g, pair) == Q.TOL_T).all() and (Q.radiance_tolerance(o, d, sc.g, pair) == Q.TOL_RADIANCE).all()
    assert (Q.radiance_tolerance(o, d, sc.g, (1, 3)) > 100 * Q.TOL_RADIANCE).all()
    G = Q.Geometry(o, d, sc.g)
    s = np.array([G.mubar[3], G.mubar[3] + 0.3, G.mubar[7] + 2 * np.sqrt(2) * G.sigma[7], 0.0])
    assert (Q.T_tolerance(o, d, s, sc.g, (1, 3)) > 2 * Q.TOL_T).tolist() == [True, False, False, False]
    assert (Q.T_tolerance(o, d, s, sc.g, (1, 4)) > 2 * Q.TOL_T).tolist() == [False, False, True, False]
    assert (Q.T_tolerance(o, d, s, sc.g, (3, 1)) > 1e-3).tolist() == [False, False, False, True]
    assert (Q.T_tolerance(o, d, s, sc.g, (2, 1)) < 2e-4).all()


def replay_steps(s, delta, most):
    """how many iterations `for (float t = 0; t <= s; t += delta)` makes: numpy's accumulate adds one float32 after the other, like the loop"""
    s, delta = np.float32(s), np.float32(delta)
    if not s >= 0:
        return 0
    with np.errstate(over="ignore"):        # (t may pass FLT_MAX: +inf ends the loop)
        t = np.add.accumulate(np.full(int(most) + 1, delta, np.float32), dtype=np.float32)
    assert t[-1] > s, "the replay needs more steps than predicted"
    return 1 + int(np.count_nonzero(t <= s))


def test_step_guard(tmp_path):
    """csrc/vrt_step_guard.hpp, compiled on its own into tests/host/step_guard.cpp: the table's rows either side of delta * 2^23, of the work
    cap, inf, NaN, negative sample points, no sample points.  For every accepted row the float32 sequence of t, replayed here, ends
    within the predicted number of steps -- the program itself runs no loop."""
    exe = str(tmp_path / "step_guard")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "simd-gaussian-ray-tracing_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "step_guard.cpp"), "-o", exe])
    args = [a for row in Q.GUARD_TABLE for a in (row[0], row[1], str(row[2]))]
    lines = subprocess.check_output([exe] + args, text=True).splitlines()
    assert len(lines) == len(Q.GUARD_TABLE)
    seen = set()
    for (s_txt, delta_txt, n, refusal), line in zip(Q.GUARD_TABLE, lines):
        word, a, rest = line.split(" ", 2)
        seen.add(refusal)
        if refusal:
            assert word == "refuse" and int(a) == refusal and rest.startswith("transmittance_step: "), (s_txt, delta_txt, n, line)
            continue
        assert word == "accept", (s_txt, delta_txt, n, line)
        steps, work = int(a), int(rest)
        delta = np.float32(float.fromhex(delta_txt) if "x" in delta_txt else float(delta_txt))
        s = np.float32([float.fromhex(v) if "x" in v else float(v) for v in s_txt.split(",")] if s_txt != "-" else [])
        assert work <= 2 ** 23
        pos = s[s >= 0]
        if not pos.size:
            assert steps == 0 and work == 0
            continue
        assert float(pos.max()) < float(delta) * 2.0 ** 23
        assert work == int(np.ceil(float(pos.max()) / float(delta))) * max(n, 1)
        ran = max(replay_steps(v, delta, steps) for v in pos)
        assert ran <= steps <= 2 * ran + 2, (s_txt, delta_txt, ran, steps)
        if pos.max() <= 1024 * delta:
            assert steps - ran <= 1, (s_txt, delta_txt, ran, steps)
    assert seen == {0, 1, 2, 3, 4}
