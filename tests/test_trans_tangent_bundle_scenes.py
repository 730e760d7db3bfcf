"""CPU checks of tests/trans_tangent_bundle_scenes.py, the model and the directions behind tests/test_gpu_trans_tangent_bundles.py: the
model is the derivative of the forward sum (T mode) and of the crossing (depth mode) along every direction, the bound is what the
float32 restatement measures, the cases and directions tell the wrong kernels from the right one, forward and reverse mode are adjoint,
and the ABI and the bindings carry the entry points."""
import copy
import os
import re

import numpy as np
import pytest

import grad_bundle_scenes as G
import ray_grad_rays_scenes as RR
import trans_grad_bundle_scenes as T
import trans_tangent_bundle_scenes as TT
from conftest import ROOT
from trans_grad_bundle_scenes import PAIRS, TGRAD_DEPTH, TGRAD_T


def small_cases(oracle, wrt):
    return [c for c in T.cases(oracle) if c.wrt == wrt and len(c.sc.g) <= 9 and c.ns <= 9]


def mid_cases(oracle):
    return [c for c in T.cases(oracle) if len(c.sc.g) <= 129 and c.ns <= 9]


def unit64(case):
    """The case with its float32 directions normalised again in float64 (test_grad_bundle_scenes.unit64 says why)"""
    out = copy.copy(case)
    out.sc = copy.copy(case.sc)
    d = case.sc.d.astype(np.float64)
    out.sc.d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out.name = case.name + " unit64"
    return out


def moved_params(base, vq, h):
    return {"mu": base["mu"] + h * vq[:, 0:3], "sigma": base["sigma"] + h * vq[:, 3], "magnitude": base["magnitude"] + h * vq[:, 4]}


def moved_rays(sc, rq, h):
    """(origins [nrays, 3], directions [nrays, 3]) in float64, every ray moved by h along its tangent: the direction along normalise(n + h t)"""
    o = np.stack([sc.origin(r).astype(np.float64) for r in range(len(sc.d))]) + h * rq[:, :3]
    return o, RR.unit64(sc.d.astype(np.float64) + h * rq[:, 3:])


def test_model_is_the_derivative_of_the_forward_sum_in_T_mode(oracle, pair="libm-libm"):
    """Central differences of the float64 T(r, s_k) along every direction -- Gaussians, rays and samples moved together, the rays along
    normalise(n + h t), kept lists held fixed -- against the model, to 1e-7 relative to S_T, with the exact erf: the model's Erf' is by
    contract the analytic one.  Step and floor are those of test_trans_grad_bundle_scenes.py's T-mode check: 1e-10 is what a difference of
    a T of size 1 with h = 1e-5 cannot see, 2^-53 / 2h = 1e-11 of rounding and h^2 / 6 = 2e-11 of its third derivative."""
    h = 1e-5
    for case in map(unit64, small_cases(oracle, TGRAD_T)):
        sc = case.sc
        names, v, rv, sd = TT.stacked(case)
        val, S = TT.model(case, pair, 1e-9, case.s, v, rv, sd)
        lists = sc.lists(1e-9, PAIRS[pair][0])
        base = T.params64(sc.g)
        s0 = np.broadcast_to(case.s.astype(np.float64), case.g.shape)
        for q, name in enumerate(names):
            vq, rq, sq = v[q].astype(np.float64), rv[q].astype(np.float64), sd[q].astype(np.float64)
            moved = []
            for sign in (+1, -1):
                p = moved_params(base, vq, sign * h)
                o, n = moved_rays(sc, rq, sign * h)
                Tm = np.ones(case.g.shape)
                for r, idx in enumerate(lists):
                    if len(idx):
                        Tm[r] = T.ray_tgrad(o[r], n[r], *T._rows(p, idx), s0[r] + sign * h * sq[r], np.ones(case.ns), TGRAD_T)[4]
                moved.append(Tm)
            fd = (moved[0] - moved[1]) / (2 * h)
            excess = np.abs(fd - val[q]) - (1e-7 * S[q] + 1e-10)
            at = np.unravel_index(np.argmax(excess), excess.shape)
            assert excess[at] <= 0, (case.name, name, at, fd[at], val[q][at], S[q][at])


def test_model_is_the_derivative_of_the_crossing_in_depth_mode(oracle, pair="libm-libm"):
    """Central differences of the depths, by float64 bisection to 1e-13, along every direction -- Gaussians, rays and LEVELS moved
    together -- against the model at the unmoved depths, to 1e-7 relative to S_T, at the levels that pass slope_ok.  The bisection
    returns the upper end of a bracket of 1e-13: up to 1e-13 / 2h of noise in a difference, 5e-10 with h = 1e-4, which is the floor; the
    h^2 term of the central difference is taken out by Richardson's step (4 f(h) - f(2h)) / 3."""
    h = 1e-4
    seen = 0
    for case in map(unit64, small_cases(oracle, TGRAD_DEPTH)):
        sc = case.sc
        lists = sc.lists(1e-9, PAIRS[pair][0])
        base = T.params64(sc.g)
        tau0 = case.tau.astype(np.float64)

        def depths(p, o, n, tau):
            m = RR.moved(sc, o, n)
            return np.stack([T.root(m, pair, r, lists[r], tau[r], g=p) for r in range(len(sc.d))])
        o0, n0 = moved_rays(sc, np.zeros((len(sc.d), 6)), 0.0)
        s0 = depths(base, o0, n0, tau0)
        live = np.isfinite(s0) & (s0 > 0)
        assert live.any() and T.slope_ok(case, pair, s0.astype(np.float32)).all(), case.name
        names, v, rv, sd = TT.stacked(case)
        val, S = TT.model(case, pair, 1e-9, s0, v, rv, sd)
        assert (val[:, ~live] == 0).all() and (S[:, ~live] == 0).all()
        for q, name in enumerate(names):
            vq, rq, sq = v[q].astype(np.float64), rv[q].astype(np.float64), sd[q].astype(np.float64)

            def central(step):
                f = [depths(moved_params(base, vq, sg * step), *moved_rays(sc, rq, sg * step), tau0 + sg * step * sq) for sg in (+1, -1)]
                return (np.where(live, f[0], 0.0) - np.where(live, f[1], 0.0)) / (2 * step)
            fd = (4 * central(h) - central(2 * h)) / 3
            excess = np.where(live, np.abs(fd - val[q]) - (1e-7 * S[q] + 5e-10), -1.0)
            at = np.unravel_index(np.argmax(excess), excess.shape)
            assert excess[at] <= 0, (case.name, name, at, fd[at], val[q][at], S[q][at])
            seen += int(live.sum())
    assert seen > 0


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_forward_and_reverse_mode_are_adjoint(oracle, pair):
    """In float64, for every case of at most 129 Gaussians and 9 samples, both modes, and every direction: sum_rk g_rk (J v)_rk, J v by the
    forward-mode restatement, equals <table(g), v> + <ray rows(g), ray v> + <grad_s(g), sample v>, all three by the transmittance
    gradient bundles' models, to 1e-12 relative to the sum of their S."""
    for case in map(unit64, mid_cases(oracle)):
        s = T.samples_of(case, pair)
        names, v, rv, sd = TT.stacked(case)
        u = case.g.astype(np.float64)
        Jv = TT.bundle_ttangent(case, pair, 1e-9, s, v, rv, sd)
        m = T.bundle_tgrad(case, pair, 1e-9, s=s, g=u)
        rows, Sr = RR.bundle_trows(case, pair, 1e-9, s=s, g=u)
        v64, rv64, sd64 = v.astype(np.float64), rv.astype(np.float64), sd.astype(np.float64)
        lhs = np.einsum("rk,drk->d", u, Jv)
        rhs = np.einsum("jc,djc->d", m.val, v64) + np.einsum("rc,drc->d", rows, rv64) + np.einsum("rk,drk->d", m.gs, sd64)
        Ssum = np.einsum("jc,djc->d", m.S, np.abs(v64)) + np.einsum("rc,drc->d", Sr, np.abs(rv64)) + np.einsum("rk,drk->d", m.Sgs, np.abs(sd64))
        for q, name in enumerate(names):
            assert abs(lhs[q] - rhs[q]) <= 1e-12 * Ssum[q], (case.name, name, lhs[q], rhs[q], Ssum[q])


def test_rho_tt(oracle):
    """RHO_TT is 4 times the worst float32 ratio measured here over every case (every ray, sample, direction and mode), and the comment
    next to it names that measurement."""
    worst = {}
    for pair in sorted(PAIRS):
        per_case = {c.name: max(TT.measured_ratio(oracle, c, pair, eps) for eps in TT.EPS) for c in T.cases(oracle)}
        top = max(per_case, key=lambda k: per_case[k][0])
        worst[pair] = per_case[top][0]
        print(pair, "worst |t32 - t64| / S_T:", per_case[top], "on", top,
              "| T mode:", max(v[0] for k, v in per_case.items() if k.startswith("T ")),
              "| depth mode:", max(v[0] for k, v in per_case.items() if k.startswith("depth ")))
        print("   ", sorted(((round(v[0] * 1e6, 2), k, v[1]) for k, v in per_case.items()), reverse=True)[:6])
    assert max(worst.values()) <= TT.RHO_TT / 4
    assert max(worst.values()) >= TT.RHO_TT / 40     # the constant is not padded either


def variant_reach(oracle, variant):
    """the most bounds by which the wrong variant moves any component of any direction of any case of at most 129 Gaussians and 9 samples"""
    best = 0.0
    for c in mid_cases(oracle):
        if (variant.startswith("depth") or variant.startswith("tau")) and c.wrt != TGRAD_DEPTH:
            continue
        s = T.samples_of(c, "vcl-as")
        _, v, rv, sd = TT.stacked(c)
        val, S = TT.model(c, "vcl-as", 1e-9, s, v, rv, sd)
        wrong = TT.bundle_ttangent(c, "vcl-as", 1e-9, s, v, rv, sd, variant=variant)
        on = S > TT.S_FLOOR
        if on.any():
            best = max(best, float((np.abs(wrong - val)[on] / TT.bound(S)[on]).max()))
    return best


def test_wrong_kernels_are_told_apart(oracle):
    """Each one-line wrong variant of ray_ttangent moves some component by more than 10 bounds: the cases and directions can see it."""
    assert len(TT.VARIANTS) >= 10
    for variant in TT.VARIANTS:
        best = variant_reach(oracle, variant)
        assert best > 10.0, (variant, best)


def test_directions_are_what_they_are_named(oracle):
    for c in T.cases(oracle):
        sc = c.sc
        dirs = {name: rest for name, *rest in TT.directions(c)}
        v, rv, sd = dirs["dense"]
        assert (v != 0).all() and (np.abs((rv[:, 3:] * sc.d).sum(1)) > 0.5).all() and sd.shape == c.g.shape and (sd != 0).all(), c.name
        for j in sc.markers:
            for col in range(TT.NCOL):
                one, none, nosd = dirs[f"one-hot {int(j)} {col}"]
                assert none is None and nosd is None and one[j, col] == 1 and np.count_nonzero(one) == 1
        assert dirs["gaussians"][1:] == [None, None] and dirs["rays"][0] is None and dirs["rays"][2] is None
        assert dirs["samples"][:2] == [None, None] and dirs["samples"][2].shape == c.g.shape
        assert dirs["samples shared"][:2] == [None, None] and dirs["samples shared"][2].shape == (c.ns,)
        assert ("origin shared" in dirs) == (sc.o.size == 3)


def test_abi_and_bindings_carry_the_transmittance_tangent_bundle(pkg):
    text = open(os.path.join(ROOT, "include", "vrt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("vrt_hip_transmittance_bundle_tangent_device", "vrt_hip_transmittance_bundle_tangent"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg.SYMBOLS
    assert callable(pkg.Renderer.transmittance_bundle_tangent) and callable(pkg.Renderer.transmittance_bundle_tangent_device)
    hpp = open(os.path.join(ROOT, "include", "vrt", "vrt.hpp")).read()
    assert "transmittance_bundle_tangent_device" in hpp and re.search(r"\bvoid transmittance_bundle_tangent\(", hpp)
