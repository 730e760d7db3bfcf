"""The scenes of tests/transmittance_bundle_scenes.py test what tests/test_gpu_transmittance_bundles.py says they test: with
oracle.transmittance alone, no GPU."""
import numpy as np
import pytest

import transmittance_bundle_scenes as S
from transmittance_bundle_scenes import RAY_PL, RAY_LCAP, TOL


def bundles(oracle, name, dim):
    g = oracle.grid_scene(dim)
    return (g,) + (S.coherent_rays(g) if name == "coherent" else S.scattered_rays(g))


@pytest.mark.parametrize("name, dim", [("coherent", 16), ("scattered", 16), ("scattered", 32)])
def test_cull_bound(oracle, name, dim):
    """What the cull drops moves T by less than 0.8 cull_eps min(N, 4096)."""
    g, o, d = bundles(oracle, name, dim)
    whole = S.oracle_T(oracle, o, d, S.PROFILE_S, g)
    culled = S.oracle_T(oracle, o, d, S.PROFILE_S, g, keep=S.kept(o, d, g))
    diff = float(np.abs(whole.astype(np.float64) - culled).max())
    print(f"{name} grid {dim}: max |T(kept) - T(whole)| = {diff:.2e}, bound {S.cull_bound(len(g)):.2e}")
    assert diff <= S.cull_bound(len(g))


@pytest.mark.parametrize("name", ["coherent", "scattered"])
def test_the_samples_see_something(oracle, name):
    """The profile's samples behind the origin (s >= 1) read attenuated rays (T < 0.95 behind the scene, at s = 8) and all but free
    ones (T > 0.99).  On the scattered rays T(8) itself spans 0.50 .. 0.987 -- every one of them crosses the grid's plane -- so the
    free readings are those of the samples before the grid; on the coherent rays T(8) alone spans 0.925 .. 0.993."""
    g, o, d = bundles(oracle, name, 16)
    T = S.oracle_T(oracle, o, d, S.PROFILE_S[1:], g)
    print(f"{name}: T(8) spans {T[:, -1].min():.3f} .. {T[:, -1].max():.3f}, T(1 .. 7) spans {T[:, :-1].min():.3f} .. {T[:, :-1].max():.3f}")
    assert (T[:, -1] < 0.95).any() and (T > 0.99).any()
    if name == "coherent":
        assert (T[:, -1] > 0.99).any()


@pytest.mark.parametrize("k", [RAY_PL - 1, RAY_PL, RAY_PL + 1])
def test_stack_markers(oracle, k):
    """The two axial rays run from T = 1 through the stack down to its optical depth of 2; its first and its last Gaussian are both
    seen, far above the tolerance the GPU test of that stack uses; the rays that miss read exactly 1."""
    g = S.stack(oracle, k)
    o, d = S.stack_rays()
    T = S.oracle_T(oracle, o, d, S.STACK_S, g)
    ax = T[:2]
    print(f"stack {k}: axial T {ax[0]}, {ax[1]}")
    assert (ax[:, 0] == 1.0).all() and (np.abs(ax[:, 1] - 0.96) < 0.01).all()
    assert ((ax[:, 2] > 0.36) & (ax[:, 2] < 0.40)).all() and ((ax[:, 3] > 0.13) & (ax[:, 3] < 0.17)).all()
    assert ((ax[:, 4] > 0.13) & (ax[:, 4] < 0.16)).all()
    assert (T[2:] == 1.0).all()
    gpu_tol = S.TOL_FULL_SUM + S.cull_bound(k) if k <= RAY_PL else TOL
    no_first = S.oracle_T(oracle, o, d, S.STACK_S, g[1:], rays=[0, 1])
    no_last = S.oracle_T(oracle, o, d, S.STACK_S, g[:-1], rays=[0, 1])
    first, last = np.abs(no_first - ax).max(1).min(), np.abs(no_last - ax)[:, 4].min()
    print(f"stack {k}: without the first {first:.2e}, without the last {last:.2e} at s = 6.5, tolerance {gpu_tol:.2e}")
    assert first >= 10 * gpu_tol and last >= 10 * gpu_tol


@pytest.mark.parametrize("n", [RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1])
def test_wide_stack_markers(oracle, n):
    """Every near-axial ray keeps the whole wide stack; each marker (0, RAY_LCAP - 1, RAY_LCAP, n - 1) moves T(8) by 500 tolerances."""
    sc = S.wide_stack(oracle, RAY_LCAP, n)
    o, d = S.wide_rays()
    assert S.kept(o, d, sc.g).all()
    T = S.oracle_T(oracle, o, d, S.WIDE_S, sc.g)
    print(f"wide stack {n}: T {T[0]}")
    assert 0.95 < T[0, 0] < 0.98 and 0.40 < T[0, 1] < 0.50 and 0.16 < T[0, 2] < 0.25    # (n = 1025: 0.966, 0.424, 0.180)
    for m in sc.markers:
        moved = np.abs(S.oracle_T(oracle, o, d, S.WIDE_S, np.delete(sc.g, m), rays=[0]) - T[0])[0, 2]
        assert moved >= 10 * TOL, (m, moved)
        assert moved >= 4e-2, (m, moved)
