"""CPU checks of tests/tangent_bundle_scenes.py, the model and the directions behind tests/test_gpu_tangent_bundles.py: the model is the
derivative of the forward sum along every direction, the bound is what the float32 restatement measures, the scenes and directions
tell ten wrong kernels from the right one, forward and reverse mode are adjoint, and the ABI carries the entry points."""
import copy
import os
import re

import numpy as np
import pytest

import grad_bundle_scenes as G
import ray_grad_rays_scenes as RR
import tangent_bundle_scenes as T
from conftest import ROOT
from grad_bundle_scenes import PAIRS


def fd_scenes(oracle):
    return [sc for sc in G.suite(oracle) if len(sc.g) <= 9]


def unit64(sc):
    """The scene with its float32 directions normalised again in float64 (test_grad_bundle_scenes.unit64 says why)"""
    out = copy.copy(sc)
    d = sc.d.astype(np.float64)
    out.d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out.name = sc.name + " unit64"
    return out


def test_model_is_the_derivative_of_the_forward_sum(oracle, pair="libm-libm"):
    """Central differences of the float64 forward sum along every direction -- Gaussians and rays moved together, the rays along
    normalise(n + h t), kept lists held fixed -- against the model, to 1e-7 relative to S_T: step and tolerance of
    test_grad_bundle_scenes.py's check, and the exact erf for its reason.
    The forward sum of a MOVED ray is G.ray_grad(..)[2] over the fixed list, the sum G.forward64 is made of (forward64 itself takes the
    scene's own rays and asks the scene for its lists); the first assertion holds the two to each other on the rays as they are.  That
    sum shares no addend with the rows under test: L is accumulated from the forward quantities before any row is."""
    ferf = G.erf
    h = 1e-5
    for sc in map(unit64, fd_scenes(oracle)):
        names, v, rv = T.stacked(sc)
        val, S = T.model(sc, pair, 1e-9, v, rv)
        lists = sc.lists(1e-9, PAIRS[pair][0])
        base = G.params64(sc.g)
        unmoved = np.zeros((len(sc.d), 4))
        for r, idx in enumerate(lists):
            if len(idx):
                unmoved[r] = G.ray_grad(sc.origin(r).astype(np.float64), sc.d[r], *G.g_rows64(base, idx), np.zeros(4), ferf=ferf)[2]
        np.testing.assert_array_equal(unmoved, G.forward64(sc, pair, 1e-9, base))
        for q, name in enumerate(names):
            vq, rq = v[q].astype(np.float64), rv[q].astype(np.float64)
            moved = []
            for sign in (+1, -1):
                p = {"albedo": base["albedo"] + sign * h * vq[:, 0:4], "mu": base["mu"] + sign * h * vq[:, 4:7],
                     "sigma": base["sigma"] + sign * h * vq[:, 7], "magnitude": base["magnitude"] + sign * h * vq[:, 8]}
                L = np.zeros((len(sc.d), 4))
                for r, idx in enumerate(lists):
                    if len(idx):
                        o = sc.origin(r).astype(np.float64) + sign * h * rq[r, :3]
                        n = RR.unit64(sc.d[r] + sign * h * rq[r, 3:])
                        L[r] = G.ray_grad(o, n, *G.g_rows64(p, idx), np.zeros(4), ferf=ferf)[2]
                moved.append(L)
            fd = (moved[0] - moved[1]) / (2 * h)
            excess = np.abs(fd - val[q]) - (1e-7 * S[q] + 1e-12)
            at = np.unravel_index(np.argmax(excess), excess.shape)
            assert excess[at] <= 0, (sc.name, name, at, fd[at], val[q][at], S[q][at])


def test_rho_t(oracle):
    """RHO_T is 4 times the worst float32 ratio measured here, and the comment next to it names that measurement."""
    worst = {}
    for pair in sorted(PAIRS):
        per_scene = {sc.name: max(T.measured_ratio(oracle, sc, pair, eps) for eps in T.EPS) for sc in G.suite(oracle)}
        print(pair, {k: f"{x:.3e}" for k, x in per_scene.items()})
        worst[pair] = max(per_scene.values())
    print("worst |t32 - t64| / S_T:", worst)
    assert max(worst.values()) <= T.RHO_T / 4
    assert max(worst.values()) >= T.RHO_T / 40     # the constant is not padded either


def test_wrong_kernels_are_told_apart(oracle):
    """Each wrong variant of ray_tangent moves some component of some scene of at most 129 kept Gaussians, along some direction, by
    more than 10 bounds."""
    scenes = [sc for sc in G.suite(oracle) if len(sc.g) <= 129]
    assert len(T.VARIANTS) >= 8
    for variant in T.VARIANTS:
        best = 0.0
        for sc in scenes:
            _, v, rv = T.stacked(sc)
            val, S = T.model(sc, "vcl-as", 1e-9, v, rv)
            wrong = T.bundle_tangent(sc, "vcl-as", 1e-9, v, rv, variant=variant)
            best = max(best, float((np.abs(wrong - val) / T.bound(S)).max()))
        assert best > 10.0, (variant, best)


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_forward_and_reverse_mode_are_adjoint(oracle, pair):
    """In float64, for every scene of at most 129 Gaussians and every direction: sum_r u_r . (J v)_r, J v by the forward-mode
    restatement, equals <table(u), v> + <ray rows(u), ray v>, table and rows by the gradient bundles' models, to 1e-12 relative to the
    sum of S.  The directions are those of unit length in float64: the two sides state the same derivative of a UNIT direction."""
    for sc in map(unit64, (sc for sc in G.suite(oracle) if len(sc.g) <= 129)):
        names, v, rv = T.stacked(sc)
        u = sc.gr.astype(np.float64)
        Jv = T.bundle_tangent(sc, pair, 1e-9, v, rv)
        table, St, _ = G.bundle_grad(sc, pair, 1e-9, gr=u)
        rows, Sr = RR.bundle_rows(sc, pair, 1e-9, gr=u)
        v64, rv64 = v.astype(np.float64), rv.astype(np.float64)
        lhs = np.einsum("rc,drc->d", u, Jv)
        rhs = np.einsum("jk,djk->d", table, v64) + np.einsum("rk,drk->d", rows, rv64)
        Ssum = np.einsum("jk,djk->d", St, np.abs(v64)) + np.einsum("rk,drk->d", Sr, np.abs(rv64))
        for q, name in enumerate(names):
            assert abs(lhs[q] - rhs[q]) <= 1e-12 * Ssum[q], (sc.name, name, lhs[q], rhs[q], Ssum[q])


def test_directions_are_what_they_are_named(oracle):
    """every column and every Gaussian in the dense direction, a ray tangent along the ray; one-hot on every marker's nine columns"""
    for sc in G.suite(oracle):
        dirs = {name: (v, rv) for name, v, rv in T.directions(sc)}
        v, rv = dirs["dense"]
        assert (v != 0).all() and (np.abs((rv[:, 3:] * sc.d).sum(1)) > 0.5).all(), sc.name
        for j in sc.markers:
            for c in range(9):
                one, none = dirs[f"one-hot {int(j)} {c}"]
                assert none is None and one[j, c] == 1 and np.count_nonzero(one) == 1
        assert dirs["albedo"][1] is None and not dirs["albedo"][0][:, 4:].any()
        assert dirs["gaussians"][1] is None and dirs["rays"][0] is None
        assert ("origin shared" in dirs) == (sc.o.size == 3)


def test_abi_declares_the_tangent_bundle(pkg):
    text = open(os.path.join(ROOT, "include", "vrt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("vrt_hip_radiance_rays_tangent_device", "vrt_hip_radiance_rays_tangent"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg.SYMBOLS
