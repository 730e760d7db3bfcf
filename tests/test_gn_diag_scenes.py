"""CPU checks of tests/gn_diag_scenes.py, the model, the bound and the scenes behind tests/test_gpu_gn_diag.py: the model is the diagonal
of an explicit J^T W J built from differences of the forward sum, the float32 restatement of the model stays within a quarter of the
bound on every scene, six wrong models miss it by ten bounds somewhere, the scenes keep the lists they are named after, and the ABI
carries the entry points."""
import copy
import os
import re

import numpy as np
import pytest

import gn_diag_scenes as D
import grad_bundle_scenes as G
from conftest import ROOT
from gn_diag_scenes import PAIRS, RAY_LCAP, RAY_PL


def unit64(sc):
    """The scene with its float32 directions normalised again in float64 (test_grad_bundle_scenes.unit64 says why)"""
    out = copy.copy(sc)
    d = sc.d.astype(np.float64)
    out.d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out.name = sc.name + " unit64"
    return out


def test_model_is_the_diagonal_of_an_explicit_JtWJ(oracle, pair="libm-libm"):
    """J [rays, 4, 9 N] from central differences of the float64 forward sum on small 5 (kept lists held fixed, the exact erf: under the
    A&S pair Erf' is by contract the analytic one), D_fd = diag(J^T W J).  The accuracy of an entry of J comes from the step alone:
      truncation: the difference at 2 h against the one at h is three times the truncation error of the latter (Richardson: the error
                  is c h^2 + O(h^4)); twice that estimate is allowed;
      rounding:   the forward sum is a few hundred float64 operations on terms of the size of the radiance: 64 * 2^-53 of the largest
                  |L| of the ray, from both evaluations, over 2 h.
    An entry of D then moves by sum w (2 |J| t + t^2)."""
    sc = unit64(D.scene(oracle, "small 5"))
    w = D.w64(sc, D.weights(sc, "seeded"))
    Dm = D.diag_of(sc, D.rows(sc, pair), w)[0]
    base = G.params64(sc.g)
    N, nrays = len(sc.g), len(sc.d)
    h = 1e-4

    def jac(step):
        J = np.zeros((nrays, 4, N, 9))
        for name, cols in G.COLS.items():
            width = base[name].shape[1] if base[name].ndim == 2 else 1
            for j in range(N):
                for c in range(width):
                    moved = []
                    for sign in (+1, -1):
                        p = {k: v.copy() for k, v in base.items()}
                        if width > 1:
                            p[name][j, c] += sign * step
                        else:
                            p[name][j] += sign * step
                        moved.append(G.forward64(sc, pair, 1e-9, p))
                    col = (cols.start + c) if isinstance(cols, slice) else cols
                    J[:, :, j, col] = (moved[0] - moved[1]) / (2 * step)
        return J
    J1, J2 = jac(h), jac(2 * h)
    Lmax = np.abs(G.forward64(sc, pair, 1e-9, base)).max(1)                                   # per ray
    t = 2.0 * np.abs(J2 - J1) / 3.0 + (2 * 64 * 2.0 ** -53 * Lmax / (2 * h))[:, None, None, None]
    ww = w[:, :, None, None]
    D_fd = (ww * J1 * J1).sum((0, 1))
    tol = (np.abs(ww) * (2 * np.abs(J1) * t + t * t)).sum((0, 1))
    keep_any = G.R.kept(sc.o, sc.d, sc.g, 1e-9, PAIRS[pair][0]).any(0)
    assert (Dm[~keep_any] == 0).all() and (D_fd[~keep_any] == 0).all()                       # a Gaussian no ray keeps: nothing, either way
    excess = np.abs(D_fd - Dm) - tol
    j = np.unravel_index(np.argmax(excess), excess.shape)
    print(f"explicit J^T W J: worst |D_fd - D| / D = {float((np.abs(D_fd - Dm)[Dm > 0] / Dm[Dm > 0]).max()):.2e}, worst tol / D = "
          f"{float((tol[Dm > 0] / Dm[Dm > 0]).max()):.2e}")
    assert excess[j] <= 0, (j, D_fd[j], Dm[j], tol[j])
    assert (tol[Dm > 0] <= 1e-4 * Dm[Dm > 0].max()).all()                                     # the differences are sharp enough to mean something
    # the albedo columns are sum_r w_rc (m V)^2: the channels do not mix
    per_ray = D.rows(sc, pair)
    for idx, v, _ in per_ray:
        for c in range(4):
            others = [k for k in range(4) if k != c]
            assert (v[c][:, others] == 0).all() and (v[others][:, :, c] == 0).all()


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_float32_restatement_stays_within_a_quarter_of_the_bound(oracle, pair):
    worst = 0.0
    for name in D.NAMES:
        sc = D.scene(oracle, name)
        for wkind in ("seeded", "null"):
            if wkind == "null" and len(sc.g) > 300:
                continue                                                                     # (the weights change no row: the long lists once)
            Dm, B, _ = D.model(sc, pair, 1e-9, wkind)
            d32 = D.restated32(oracle, sc, pair, 1e-9, D.weights(sc, wkind)).astype(np.float64)
            assert (d32[B == 0] == 0).all() and (Dm[B == 0] == 0).all()                       # B = 0: a row no ray keeps
            ratio = np.abs(d32 - Dm) / np.where(B > 0, B, 1.0)
            worst = max(worst, float(ratio.max()))
            j = np.unravel_index(np.argmax(ratio), ratio.shape)
            assert ratio[j] <= 0.25, (name, wkind, j, d32[j], Dm[j], B[j])
    print(f"{pair}: worst |D32 - D64| / B = {worst:.3f}")


def test_wrong_models_are_told_apart(oracle):
    """Each of the six wrong models misses the model by at least 10 B on some entry of some scene"""
    scenes = [D.scene(oracle, n) for n in D.NAMES if "wide" not in n]
    for which in D.WRONG:
        best = 0.0
        for sc in scenes:
            Dm, B, _ = D.model(sc, "vcl-as", 1e-9, "seeded")
            wrong = D.wrong_model(sc, "vcl-as", 1e-9, D.weights(sc, "seeded"), which)
            best = max(best, float((np.abs(wrong - Dm)[B > 0] / B[B > 0]).max()))
        assert best >= 10.0, (which, best)


def test_bound_is_small_where_the_diagonal_is_not(oracle):
    """A condition on scenes and bound: on every marker Gaussian the bound of each entry is at most 1e-3 of the row's largest entry"""
    for name in D.NAMES:
        sc = D.scene(oracle, name)
        for ordered in (False, True):
            Dm, B, _ = D.model(sc, "vcl-as", 1e-9, "seeded", ordered)
            for j in sc.markers:
                assert B[j].max() <= 1e-3 * Dm[j].max(), (name, j, B[j].max(), Dm[j].max())


def test_scenes_keep_the_lists_they_are_named_after(oracle):
    for eps in G.EPS:
        for ek in (0, 1):
            assert [len(l) for l in D.scene(oracle, f"stack {RAY_PL + 1}|{RAY_PL + 2}").lists(eps, ek)] == [RAY_PL + 2, RAY_PL + 1]
            assert [len(l) for l in D.scene(oracle, f"stack {RAY_PL}|{RAY_PL + 1}").lists(eps, ek)] == [RAY_PL + 1, RAY_PL]
            assert [len(l) for l in D.scene(oracle, f"wide {RAY_LCAP}").lists(eps, ek)] == [RAY_LCAP]
    assert sorted(D.NAMES) == sorted(sc.name for sc in D.suite(oracle))
    for name in D.NAMES:
        sc = D.scene(oracle, name)
        w = D.weights(sc, "seeded")
        assert w.shape == (len(sc.d), 4) and w.dtype == np.float32 and w.min() >= 0.25 and w.max() <= 4.0
        assert D.weights(sc, "null") is None


def test_abi_declares_the_diagonal_bundle(pkg):
    text = open(os.path.join(ROOT, "include", "vrt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("vrt_hip_radiance_rays_gn_diag_device", "vrt_hip_radiance_rays_gn_diag"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg.SYMBOLS
    assert hasattr(pkg.Renderer, "radiance_rays_gn_diag") and hasattr(pkg.Renderer, "radiance_rays_gn_diag_device")
