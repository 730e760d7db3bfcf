"""CPU checks of tests/trans_grad_bundle_scenes.py, the model and the cases behind tests/test_gpu_trans_grad_bundles.py: the model is
the derivative of its forward sum in both modes, the forward sum is the oracle's T, the bound is what the float32 restatement measures,
the cases tell ten wrong models from the right one, the depth-mode levels meet the slope condition, the scenes keep the lists they are
named after, and the ABI carries the entry points."""
import copy
import os
import re

import numpy as np
import pytest

import grad_bundle_scenes as G
import trans_grad_bundle_scenes as S
import transmittance_bundle_scenes as TB
from conftest import ROOT
from trans_grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL, TGRAD_DEPTH, TGRAD_T


def small_cases(oracle, wrt):
    return [c for c in S.cases(oracle) if c.wrt == wrt and len(c.sc.g) <= 9 and c.ns <= 9]


def unit64(case):
    """The case with its float32 directions normalised again in float64 (test_grad_bundle_scenes.unit64 says why)"""
    out = copy.copy(case)
    out.sc = copy.copy(case.sc)
    d = case.sc.d.astype(np.float64)
    out.sc.d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out.name = case.name + " unit64"
    return out


def differences(case, loss, base, names, h=1e-5):
    """{(name, j, c): central difference of loss(params) in component c of row j of params[name]} over the Gaussians some ray keeps"""
    keep_any = G.R.kept(case.sc.o, case.sc.d, case.sc.g, 1e-9, 0).any(0)
    out = {}
    for name in names:
        width = base[name].shape[1] if base[name].ndim == 2 else 1
        for j in np.nonzero(keep_any)[0]:
            for c in range(width):
                moved = []
                for sign in (+1, -1):
                    p = {k: v.copy() for k, v in base.items()}
                    if width > 1:
                        p[name][j, c] += sign * h
                    else:
                        p[name][j] += sign * h
                    moved.append(loss(p))
                out[name, j, c] = (moved[0] - moved[1]) / (2 * h)
    return out


COL = {"mu": 0, "sigma": 3, "magnitude": 4}


def test_model_is_the_derivative_of_its_forward_sum_in_T_mode(oracle, pair="libm-libm"):
    """Central differences of the float64 forward sum sum_k g_k T_k (kept lists held fixed) against the model, to 1e-7 relative to S, in
    mu, sigma, magnitude and s -- with the exact erf: the model's Erf' is by contract the analytic one.  The floor of 1e-10 is what a
    difference of a sum of size 1 with h = 1e-5 cannot see: 2^-53 / 2h = 1e-11 of rounding and h^2 / 6 = 2e-11 of its third derivative."""
    for case in map(unit64, small_cases(oracle, TGRAD_T)):
        m = S.bundle_tgrad(case, pair, 1e-9)
        g = case.g.astype(np.float64)
        base = S.params64(case.sc.g)
        fd = differences(case, lambda p: (S.bundle_tgrad(case, pair, 1e-9, params=p).T * g).sum(), base, COL)
        for (name, j, c), v in fd.items():
            col = COL[name] + c
            assert abs(v - m.val[j, col]) <= 1e-7 * m.S[j, col] + 1e-10, (case.name, name, j, c, v, m.val[j, col], m.S[j, col])
        # d / d s: per ray and sample (a shared sample: the per-ray outputs summed)
        s0 = np.broadcast_to(case.s.astype(np.float64), g.shape).copy()
        h = 1e-5
        for r in range(g.shape[0]):
            for k in range(g.shape[1]):
                moved = []
                for sign in (+1, -1):
                    s = s0.copy()
                    s[r, k] += sign * h
                    moved.append((S.bundle_tgrad(case, pair, 1e-9, s=s, rays=[r]).T[r] * g[r]).sum())
                v = (moved[0] - moved[1]) / (2 * h)
                assert abs(v - m.gs[r, k]) <= 1e-7 * m.Sgs[r, k] + 1e-10, (case.name, "s", r, k, v, m.gs[r, k])


def test_model_is_the_derivative_of_the_crossing_in_depth_mode(oracle, pair="libm-libm"):
    """Central differences of sum_k g_k depth_k, the depths by float64 bisection to 1e-13, against the model at those depths, in mu,
    sigma, magnitude and tau.  The bisection leaves 1e-13 / 2h = 5e-9 of noise per sample in a difference: 1e-6 S + 1e-7."""
    for case in map(unit64, small_cases(oracle, TGRAD_DEPTH)):
        sc = case.sc
        lists = sc.lists(1e-9, 0)
        g = case.g.astype(np.float64)

        def depths(p=None, tau=None):
            tau = case.tau if tau is None else tau
            return np.stack([S.root(sc, pair, r, lists[r], tau[r], g=p) for r in range(len(sc.d))])
        s0 = depths()
        live = np.isfinite(s0) & (s0 > 0)
        assert live.any(), case.name

        def loss(p=None, tau=None):
            return (np.where(live, depths(p, tau), 0.0) * g).sum()
        m = S.bundle_tgrad(case, pair, 1e-9, s=s0)
        fd = differences(case, loss, S.params64(sc.g), COL)
        for (name, j, c), v in fd.items():
            col = COL[name] + c
            assert abs(v - m.val[j, col]) <= 1e-6 * m.S[j, col] + 1e-7, (case.name, name, j, c, v, m.val[j, col], m.S[j, col])
        h = 1e-5
        for r, k in zip(*np.nonzero(live)):
            moved = []
            for sign in (+1, -1):
                tau = case.tau.astype(np.float64).copy()
                tau[r, k] += sign * h
                moved.append(loss(tau=tau))
            v = (moved[0] - moved[1]) / (2 * h)
            assert abs(v - m.gs[r, k]) <= 1e-6 * m.Sgs[r, k] + 1e-7, (case.name, "tau", r, k, v, m.gs[r, k])
        assert (m.gs[~live] == 0).all()


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_forward_sum_is_the_oracles_T(oracle, pair):
    """What is differentiated is what transmittance_bundle computes: the oracle's T over the kept rows of the same rays, up to float32."""
    ek, fk = PAIRS[pair]
    for case in small_cases(oracle, TGRAD_T):
        sc = case.sc
        T = S.bundle_tgrad(case, pair, 1e-9, g=np.ones_like(case.g)).T
        want = TB.oracle_T(oracle, sc.o, sc.d, case.s, sc.g, ek, fk, keep=sc.lists(1e-9, ek))
        assert np.abs(T - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), case.name


def test_rho(oracle):
    """RHO_T is 4 times the worst float32 ratio measured here over every case (every ray, sample set and mode), and the comment next to
    it names that measurement."""
    worst = {}
    for pair in sorted(PAIRS):
        per_case = {c.name: max(S.measured_ratio(oracle, c, pair, eps) for eps in S.EPS) for c in S.cases(oracle)}
        top = max(per_case, key=per_case.get)
        worst[pair] = per_case[top]
        print(pair, "worst |g32 - g64| / S:", per_case[top], "on", top,
              "| T mode:", max(v for k, v in per_case.items() if k.startswith("T ")), "| depth mode:", max(v for k, v in per_case.items() if k.startswith("depth ")))
        print("   ", sorted(((round(v * 1e6, 2), k) for k, v in per_case.items()), reverse=True)[:6])
    assert max(worst.values()) <= S.RHO_T / 4
    assert max(worst.values()) >= S.RHO_T / 40     # the constant is not padded either


def test_wrong_models_are_told_apart(oracle):
    """Each wrong variant moves some marker component of some case of at most 129 Gaussians by at least 10 B."""
    cs = [c for c in S.cases(oracle) if len(c.sc.g) <= 129 and c.ns <= 9]
    for variant in S.VARIANTS:
        best = 0.0
        for c in cs:
            if variant.startswith("depth") and c.wrt != TGRAD_DEPTH:
                continue
            s = S.samples_of(c, "vcl-as")
            right = S.bundle_tgrad(c, "vcl-as", 1e-9, s=s)
            wrong = S.bundle_tgrad(c, "vcl-as", 1e-9, s=s, variant=variant).val
            m = c.sc.markers
            B = S.bound(right.S[m])
            on = right.S[m] > S.S_FLOOR
            if on.any():
                best = max(best, float((np.abs(wrong[m] - right.val[m])[on] / B[on]).max()))
        assert best >= 10.0, (variant, best)


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_depth_levels_meet_the_slope_condition(oracle, pair):
    """Every live sample of a depth-mode case sits where T |S| >= SLOPE_MIN; the cases hold live samples, +inf and 0 depths."""
    seen = np.zeros(3, bool)
    for c in S.cases(oracle):
        if c.wrt != TGRAD_DEPTH:
            continue
        d = S.model_depths(c, pair)
        assert S.slope_ok(c, pair, d).all(), c.name
        live = np.isfinite(d) & (d > 0)
        assert live.any(), c.name
        seen |= [live.any(), np.isinf(d).any(), (d == 0).any()]
    assert seen.all()


def test_scenes_keep_the_lists_they_are_named_after(oracle):
    for eps in S.EPS:
        for ek in (0, 1):
            for mode in ("T", "depth"):
                assert [len(l) for l in S.case(oracle, f"{mode} stack {RAY_PL}|{RAY_PL + 1}").sc.lists(eps, ek)] == [RAY_PL + 1, RAY_PL]
                assert [len(l) for l in S.case(oracle, f"{mode} {S.CHUNK_SCENE} ns={S.NSC}").sc.lists(eps, ek)] == [RAY_PL + 1, RAY_PL]
                assert [len(l) for l in S.case(oracle, f"{mode} wide {RAY_LCAP + 1}").sc.lists(eps, ek)] == [RAY_LCAP + 1]
    sca = S.case(oracle, "T grid16 scattered").sc
    coh = S.case(oracle, "T grid16 coherent").sc
    assert max(len(l) for l in sca.lists()) > RAY_PL >= max(len(l) for l in coh.lists())     # both kernels; the coherent bundle all short
    assert sorted({c.ns for c in S.cases(oracle) if "small 9 ns=" in c.name}) == sorted(S.SAMPLE_COUNTS)
    assert {c.name for c in S.cases(oracle)} == {f"{m} {n}" for m in ("T", "depth") for n in S.PARITY}


def test_samples_lie_before_inside_and_behind(oracle):
    """A T-mode case of three samples or more has one at the origin, one inside and one behind what each ray keeps."""
    for c in S.cases(oracle):
        if c.wrt != TGRAD_T or c.ns < 3:
            continue
        for r, idx in enumerate(c.sc.lists()):
            if len(idx) and c.s.ndim == 2:
                lo, hi = S.extent(c.sc, r, idx)
                s = c.samples(r)
                assert s.min() <= max(lo, 0.0) and ((s > lo) & (s < hi)).any() and s.max() > hi, (c.name, r)


def test_abi_declares_the_transmittance_gradient_bundle(pkg):
    text = open(os.path.join(ROOT, "include", "vrt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("vrt_hip_transmittance_bundle_grad_device", "vrt_hip_transmittance_bundle_grad"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg.SYMBOLS
    assert re.search(r"VRT_HIP_TGRAD_T\s*=\s*0\b", text) and re.search(r"VRT_HIP_TGRAD_DEPTH\s*=\s*1\b", text)
    assert (pkg.TGRAD_T, pkg.TGRAD_DEPTH) == (0, 1) == (TGRAD_T, TGRAD_DEPTH)
