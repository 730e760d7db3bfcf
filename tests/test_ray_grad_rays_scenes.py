"""CPU checks of tests/ray_grad_rays_scenes.py, the model and the scenes behind tests/test_gpu_ray_grad_rays.py: the model is the
derivative of the float64 forward sums along the origin and along two tangents of the direction, its direction rows are perpendicular
to the direction, the bound is what the float32 restatement measures, the scenes tell the wrong models from the right one on rays on
which the bound is small, the pose fit's steps lower the model's loss, and the ABI carries the entry points."""
import os
import re

import numpy as np
import pytest

import ray_grad_rays_scenes as S
from conftest import ROOT
from ray_grad_rays_scenes import G, PAIRS, RAY_LCAP, RAY_PL, T

H = 1e-5
SMALL = [f"small {n}" for n in (1, 2, 3, 5, 9)]


def directions(n):
    """what a ray is moved along: the three axes of the origin, two tangents of the direction -- (is it the direction, vector, columns of the row)"""
    t1, t2 = S.tangents(n)
    return [(False, np.eye(3)[a], slice(0, 3)) for a in range(3)] + [(True, t, slice(3, 6)) for t in (t1, t2)]


def check_derivative(name, r, row, Srow, o, n, loss):
    """central differences of loss(o, n) at h = 1e-5 against the row, to 1e-7 S + 1e-12"""
    for is_dir, t, cols in directions(n):
        f = [loss(o, S.unit64(n + s * H * t)) if is_dir else loss(o + s * H * t, n) for s in (+1, -1)]
        fd = (f[0] - f[1]) / (2 * H)
        got, tol = float(row[cols] @ t), 1e-7 * float(Srow[cols] @ np.abs(t)) + 1e-12
        assert abs(fd - got) <= tol, (name, r, is_dir, t, fd, got, tol)


def test_radiance_rows_are_the_derivative_of_the_forward_sum(oracle, pair="libm-libm"):
    for sc in (s for s in S.suite(oracle) if len(s.g) <= 9):
        lists = sc.lists(1e-9, PAIRS[pair][0])
        for r in range(len(sc.d)):
            o, n = sc.origin(r).astype(np.float64), S.unit64(sc.d[r])
            row, Srow = S.ray_rows(o, n, *G.g_rows64(G.params64(sc.g), lists[r]), sc.gr[r].astype(np.float64))
            check_derivative(sc.name, r, row, Srow, o, n, lambda o_, n_: S.radiance_loss(sc, pair, lists, r, o_, n_))


@pytest.mark.parametrize("mode", ["T", "depth"])
def test_transmittance_and_depth_rows_are_the_derivative_of_the_forward_sum(oracle, mode, pair="libm-libm"):
    """T mode: of sum_k g_k T(s_k) (T.forward_T); depth mode: of sum_k g_k depth(tau_k), the float64 crossing (T.root)"""
    for name in SMALL:
        case = T.case(oracle, f"{mode} {name}")
        sc = case.sc
        lists = sc.lists(1e-9, PAIRS[pair][0])
        p64 = T.params64(sc.g)
        for r in range(len(sc.d)):
            idx = lists[r]
            o, n = sc.origin(r).astype(np.float64), S.unit64(sc.d[r])
            g = case.g[r].astype(np.float64)

            def forward(o_, n_):
                m = S.moved(sc, o_, n_[None, :])
                if mode == "T":
                    return T.forward_T(m, pair, 0, idx, case.samples(r).astype(np.float64), p64)
                return T.root(m, pair, 0, idx, case.tau[r].astype(np.float64), p64)
            s = forward(o, n)
            live = np.isfinite(s) & (s > 0) if mode == "depth" else np.ones(len(s), bool)
            if mode == "T":
                s = case.samples(r).astype(np.float64)
            row, Srow = S.ray_trows(o, n, *T._rows(p64, idx), np.where(live, s, 0.0), np.where(live, g, 0.0), case.wrt)
            check_derivative(case.name, r, row, Srow, o, n, lambda o_, n_: float((np.where(live, forward(o_, n_), 0.0) * g).sum()))


def test_direction_rows_are_perpendicular_to_the_direction(oracle, pair="vcl-as"):
    """g_n . n <= 1e-12 S, with the float32 directions normalised again in float64 (a float32 one is 6e-8 off unit length)"""
    def check(name, r, n, row, Srow):
        assert abs(row[3:] @ n) <= 1e-12 * (Srow[3:] @ np.abs(n)), (name, r, row[3:] @ n)
    for sc in S.suite(oracle):
        for r, idx in enumerate(sc.lists(1e-9, PAIRS[pair][0])):
            if len(idx):
                n = S.unit64(sc.d[r])
                check(sc.name, r, n, *S.ray_rows(sc.origin(r).astype(np.float64), n, *G.g_rows64(sc.g, idx), sc.gr[r], ferf=G.erf_as))
    for case in [T.case(oracle, f"{m} {n}") for m in ("T", "depth") for n in SMALL + ["grid16 scattered"]]:
        sc, s = case.sc, T.samples_of(case, pair)
        for r, idx in enumerate(sc.lists(1e-9, PAIRS[pair][0])):
            if len(idx):
                n = S.unit64(sc.d[r])
                check(case.name, r, n, *S.ray_trows(sc.origin(r).astype(np.float64), n, *T._rows(sc.g, idx), case.samples(r, s), case.g[r], case.wrt,
                                                    ferf=G.erf_as))


def test_rho_r(oracle):
    """RHO_R is 4 times the worst float32 ratio measured here, and the comment next to it names that measurement."""
    worst = {}
    wide = [S.wide_off_axis_case(oracle, m) for m in ("T", "depth")]
    for pair in sorted(PAIRS):
        worst[pair] = max([S.measured_ratio(oracle, sc, pair, eps) for sc in S.suite(oracle) for eps in S.EPS]
                          + [S.measured_tratio(oracle, c, pair, eps) for c in T.cases(oracle) + wide for eps in S.EPS])
    print("worst |g32 - g64| / S:", worst)
    assert max(worst.values()) <= S.RHO_R / 4
    assert max(worst.values()) >= S.RHO_R / 40     # the constant is not padded either


def worst_move(rows, Ssum, wrong, marker):
    B = S.bound(Ssum[marker])
    return float((np.abs(wrong[marker] - rows[marker]) / B).max()) if marker.any() else 0.0


def test_wrong_radiance_models_are_told_apart(oracle):
    """Each wrong variant moves some component of some marker ray's row by at least 10 B (scenes of at most 129 Gaussians kept)."""
    scenes = [sc for sc in S.suite(oracle) if len(sc.g) <= 129]
    for variant in S.VARIANTS:
        best = 0.0
        for sc in scenes:
            rows, Ssum = S.model(sc, "vcl-as")
            wrong = S.bundle_rows(sc, "vcl-as", 1e-9, variant=variant)[0]
            best = max(best, worst_move(rows, Ssum, wrong, S.is_marker(rows, Ssum)))
        assert best >= 10.0, (variant, best)


def test_wrong_transmittance_models_are_told_apart(oracle):
    names = SMALL + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64)]
    for variant in S.T_VARIANTS:
        best = 0.0
        for mode in (["depth"] if variant == "depth_sign" else ["T", "depth"]):
            for name in names:
                case = T.case(oracle, f"{mode} {name}")
                rows, Ssum = S.tmodel(case, "vcl-as")
                wrong = S.bundle_trows(case, "vcl-as", 1e-9, s=T.samples_of(case, "vcl-as"), variant=variant)[0]
                best = max(best, worst_move(rows, Ssum, wrong, S.is_marker(rows, Ssum)))
        assert best >= 10.0, (variant, best)


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_marker_rays(oracle, pair):
    """On a marker ray the bound of every component is at most 1e-3 of the row's largest component: every ray of the small scenes, the
    stacks, the coherent grid bundle and the off-axis wide ray, at least 95 % of the scattered grid bundle's; and of the transmittance
    cases' rays whose row is not zero, all in the small scenes, the stacks and on the wide ray, 95 % of either grid bundle's."""
    for eps in S.EPS:
        for sc in S.suite(oracle):
            m = S.is_marker(*S.model(sc, pair, eps))
            assert m.mean() >= (0.95 if sc.name == "grid16 scattered" else 1.0), (sc.name, eps, m.mean())
        names = SMALL + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64)] + ["grid16 coherent", "grid16 scattered"]
        for mode in ("T", "depth"):
            for case in [T.case(oracle, f"{mode} {n}") for n in names] + [S.wide_off_axis_case(oracle, mode)]:
                rows, Ssum = S.tmodel(case, pair, eps)
                nz = np.abs(rows).max(1) > 0
                assert nz.any(), case.name
                m = S.is_marker(rows[nz], Ssum[nz])
                assert m.mean() >= (0.95 if "grid16" in case.name else 1.0), (case.name, eps, m.mean())


def test_the_off_axis_ray_keeps_the_whole_stack(oracle):
    sc = S.wide_off_axis(oracle)
    assert len(sc.d) == 1 and not G.undecided(sc.o, sc.d, sc.g).any()
    axial = G.scene(oracle, f"wide {RAY_LCAP + 1}").d[0]
    assert np.abs(sc.d[0] - axial).max() > 1e-3
    for eps in S.EPS:
        for ek in (0, 1):
            assert [len(l) for l in sc.lists(eps, ek)] == [RAY_LCAP + 1]
    assert S.is_marker(*S.model(sc, "vcl-as")).all()


def test_abi_declares_the_ray_gradients(pkg):
    text = open(os.path.join(ROOT, "include", "vrt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("vrt_hip_radiance_rays_grad_rays_device", "vrt_hip_radiance_rays_grad_rays", "vrt_hip_transmittance_bundle_grad_rays_device",
                 "vrt_hip_transmittance_bundle_grad_rays"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg.SYMBOLS
    assert re.search(r"VRT_HIP_RAY_GRAD_STRIDE\s*=\s*8\b", text) and pkg.RAY_GRAD_STRIDE == 8 == S.RAY_GRAD_STRIDE


def test_pose_fit_lowers_the_models_loss(oracle):
    """64 rays of a pinhole camera on `small 9`, started 0.05 units and 1 degree off: the fixed plain gradient steps of PoseFit lower the
    float64 model's loss by at least a factor of 10."""
    fit = S.PoseFit(oracle)
    assert abs(np.linalg.norm(fit.T0) - 0.05) < 1e-6 and abs(np.linalg.norm(fit.W0) - np.deg2rad(1.0)) < 1e-12
    assert len(fit.d0) == 64
    losses = fit.run()
    print("pose fit, model:", losses)
    assert losses[0] > 0 and losses[-1] <= losses[0] / 10
