"""CPU checks of tests/grad_bundle_scenes.py, the model and the scenes behind tests/test_gpu_grad_bundles.py: the model is the
derivative of its forward sum, the forward sum is the library's radiance, the bound is what the float32 restatement measures, the
scenes tell ten wrong models from the right one and keep the lists they are named after, and the ABI carries the entry points."""
import copy
import os
import re

import numpy as np
import pytest

import grad_bundle_scenes as S
from conftest import ROOT
from grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL


def fd_scenes(oracle):
    return [sc for sc in S.suite(oracle) if len(sc.g) <= 9]


def unit64(sc):
    """The scene with its float32 directions normalised again in float64: the formulas are those of a UNIT direction (a float32 one is
    6e-8 off, which the differences of the forward sum see at 1e-7 of S and the bound never does)."""
    out = copy.copy(sc)
    d = sc.d.astype(np.float64)
    out.d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out.name = sc.name + " unit64"
    return out


def test_model_is_the_derivative_of_its_forward_sum(oracle, pair="libm-libm"):
    """Central differences of the float64 forward sum (kept lists held fixed) against the model, to 1e-7 relative to S -- with the
    exact erf: under the A&S pair the model's Erf' is by contract the analytic one, which is not the slope of the A&S form."""
    for sc in map(unit64, fd_scenes(oracle)):
        val, Ssum = S.model(sc, pair)
        keep_any = S.R.kept(sc.o, sc.d, sc.g, 1e-9, PAIRS[pair][0]).any(0)
        base = S.params64(sc.g)
        gr = sc.gr.astype(np.float64)
        h = 1e-5
        for name, cols in S.COLS.items():
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
                        moved.append((S.forward64(sc, pair, 1e-9, p) * gr).sum())
                    fd = (moved[0] - moved[1]) / (2 * h)
                    col = (cols.start + c) if isinstance(cols, slice) else cols
                    assert abs(fd - val[j, col]) <= 1e-7 * Ssum[j, col] + 1e-12, (sc.name, name, j, c, fd, val[j, col], Ssum[j, col])


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_forward_sum_is_the_librarys_radiance(oracle, pair):
    """What is differentiated is what radiance_rays computes: the oracle's radiance of the same rays, up to the cull and float32."""
    ek, fk = PAIRS[pair]
    for sc in fd_scenes(oracle):
        L = S.forward64(sc, pair, 0.0)
        want = S.R.oracle_radiance(oracle, sc.o, sc.d, sc.g, ek, fk)
        assert np.abs(L - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), sc.name


def test_rho(oracle):
    """RHO is 4 times the worst float32 ratio measured here, and the comment next to it names that measurement."""
    worst = {}
    for pair in sorted(PAIRS):
        worst[pair] = max(S.measured_ratio(oracle, sc, pair, eps) for sc in S.suite(oracle) for eps in S.EPS)
    print("worst |g32 - g64| / S:", worst)
    assert max(worst.values()) <= S.RHO / 4
    assert max(worst.values()) >= S.RHO / 40     # the constant is not padded either


def test_wrong_models_are_told_apart(oracle):
    """Each wrong variant moves some marker component of some scene of at most 129 kept Gaussians by at least 10 B."""
    scenes = [sc for sc in S.suite(oracle) if len(sc.g) <= 129]
    for variant in S.VARIANTS:
        best = 0.0
        for sc in scenes:
            val, Ssum = S.model(sc, "vcl-as")
            wrong = S.bundle_grad(sc, "vcl-as", 1e-9, variant=variant)[0]
            m = sc.markers
            B = S.bound(Ssum[m])
            on = B > 0
            if on.any():
                best = max(best, float((np.abs(wrong[m] - val[m])[on] / B[on]).max()))
        assert best >= 10.0, (variant, best)


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_bound_is_small_on_the_markers(oracle, pair):
    """A condition on the scenes: on every marker Gaussian the bound of each component is at most 1e-3 of its largest component."""
    for sc in S.suite(oracle):
        for eps in S.EPS:
            val, Ssum = S.model(sc, pair, eps)
            for j in sc.markers:
                assert S.bound(Ssum[j]).max() <= 1e-3 * np.abs(val[j]).max(), (sc.name, eps, j, S.bound(Ssum[j]).max(), np.abs(val[j]).max())


def test_scenes_keep_the_lists_they_are_named_after(oracle):
    for eps in S.EPS:
        for ek in (0, 1):
            for k in (RAY_PL, 64, 128):
                assert [len(l) for l in S.scene(oracle, f"stack {k}|{k + 1}").lists(eps, ek)] == [k + 1, k]
            assert [len(l) for l in S.scene(oracle, f"wide {RAY_LCAP + 1}").lists(eps, ek)] == [RAY_LCAP + 1]
            for n in (5, 9):
                sc = S.small(oracle, n)
                keep = S.R.kept(sc.o, sc.d, sc.g, eps, ek)
                assert not keep[:, 1].any() and keep[:, 2].all() and keep[:, 3].all(), n   # magnitude 0 dropped; negative, behind kept
    coh, sca = S.scene(oracle, "grid16 coherent"), S.scene(oracle, "grid16 scattered")
    assert len(coh.g) >= 0.95 * 256 and len(sca.g) >= 0.95 * 256
    assert max(len(l) for l in sca.lists()) > RAY_PL >= max(len(l) for l in coh.lists())     # both kernels; the coherent bundle all short


def test_abi_declares_the_gradient_bundle(pkg):
    text = open(os.path.join(ROOT, "include", "vrt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("vrt_hip_radiance_rays_grad_device", "vrt_hip_radiance_rays_grad"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg.SYMBOLS
    assert re.search(r"VRT_HIP_GRAD_STRIDE\s*=\s*12\b", text) and pkg.GRAD_STRIDE == 12
