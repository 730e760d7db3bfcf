"""The scenes, levels and tolerances of tests/depth_bundle_scenes.py test what tests/test_gpu_depth_bundles.py says they test: with
the oracle and the float64 model alone, no GPU.

Figures of the stacks (ray_bundle_scenes.stack(k), k = 31 / 32 / 33, the axial ray), from the model and from oracle.transmittance:
T_inf = exp(-2) = 0.135 (a Gaussian's weight is sigma cbar K with K = 1 / 0.79788 = 1.2533, so the stack's optical depth is 2, as
test_transmittance_bundle_scenes.py::test_stack_markers reads it: T(6.5) = 0.135); roots 4.260 / 4.411 / 4.596 / 4.668 at tau = 0.9 /
0.75 / 0.6 / 0.55; tau = 0.5 has the root 4.746 and tau = 0.1 is a miss; dropping Gaussian 0 moves every root by 0.05 .. 0.06; the last
Gaussian sits at s = 5.8 and does not move the tau = 0.55 root (< 1e-9), so the marker level is 0.15, where dropping it moves the root
by 8e-3 .. 9e-3.  (T_inf = 0.529 with roots 4.447 .. 5.725 would be the same stack with a weight of sigma cbar / sqrt(2 pi).)"""
import math

import numpy as np
import pytest

import depth_bundle_scenes as S
from depth_bundle_scenes import RAY_PL, RAY_LCAP, TOL, MARKER_FACTOR


def stack_tol(k):
    return S.TOL_FULL_SUM + S.cull_bound(k) if k <= RAY_PL else TOL


@pytest.mark.parametrize("pair", [(0, 0), (1, 1)])
def test_the_model_is_the_oracle(oracle, pair):
    """T(s) of the model over a ray's kept Gaussians is oracle.transmittance over the whole scene under the same (Exp, Erf) pair, within
    the float32 oracle's rounding and the cull bound."""
    g = oracle.grid_scene(16)
    o, d = S.scattered_rays(g)
    s = np.linspace(0.0, 8.0, 17).astype(np.float32)
    mods = S.models(o, d, g, erf_kind=pair[1])
    ref = S.oracle_T(oracle, o, d, s, g, pair[0], pair[1])
    got = np.array([[mods[r].T(float(v)) for v in s] for r in range(len(d))])
    print(f"max |model - oracle| = {np.abs(got - ref).max():.2e}")
    assert np.abs(got - ref).max() <= S.TOL_FULL_SUM + S.cull_bound(len(g))
    m = mods[0]
    for v in (2.0, 3.5, 4.0):                                   # the closed-form slope against a central difference
        num = (m.T(v - 1e-5) - m.T(v + 1e-5)) / 2e-5
        assert abs(m.slope(v) - num) <= 1e-6 + (1e-5, 2e-2)[pair[1]] * abs(num)    # (the A&S form's own derivative: within 2 % of erf's)
    assert all(abs(x.T(x.s_end) - x.T_inf) <= (1e-15, 1e-8)[pair[1]] for x in mods.values())       # every Erf is saturated at s_end


@pytest.mark.parametrize("k", [RAY_PL - 1, RAY_PL, RAY_PL + 1])
def test_stack_figures_and_markers(oracle, k):
    g = S.stack(oracle, k)
    o, d = S.stack_rays()
    mods = S.models(o, d, g)
    ax = mods[0]
    roots = [ax.root(t) for t in S.STACK_LEVELS]
    print(f"stack {k}: T_inf {ax.T_inf:.4f}, s_end {ax.s_end:.3f}, roots {roots}, root(0.5) {ax.root(0.5)}")
    assert abs(ax.T_inf - math.exp(-2.0)) < 1e-3
    assert np.abs(np.array(roots) - [4.260, 4.411, 4.596, 4.668]).max() < 2e-3
    assert abs(ax.root(0.5) - 4.746) < 2e-3 and ax.root(S.STACK_MISS_LEVEL) is None and mods[1].root(S.STACK_MISS_LEVEL) is None
    assert all(len(mods[r].w) == 0 and mods[r].T_inf == 1.0 and mods[r].s_end == 0.0 for r in range(2, 64))     # the wave-mates keep nothing
    for t, root in zip(S.STACK_LEVELS, roots):                  # the oracle reads the level at the model's root
        assert abs(float(oracle.transmittance(o, d[0], np.float32(root), g, 0, 0)[0]) - float(t)) <= 1e-5
        moved = S.RayModel(o, d[0], g[1:]).root(t) - root
        assert 0.045 <= moved <= 0.065, (float(t), moved)
    assert abs(S.RayModel(o, d[0], g[:-1]).root(S.STACK_LEVELS[-1]) - roots[-1]) < 1e-6    # the last Gaussian is not seen at 0.55 ...
    for r in (0, 1):                                            # ... but at the marker levels both ends are, far above the s-tolerance
        lvl, m = S.STACK_MARKER_LEVELS[r], mods[r]
        root, tol_s = m.root(lvl), S.s_tolerance(m, lvl, stack_tol(k))
        assert root is not None and tol_s is not None and lvl - m.T_inf < 0.02
        for name, rows in (("first", g[1:]), ("last", g[:-1])):
            other = S.RayModel(o, d[r], rows).root(lvl)
            moved = math.inf if other is None else abs(other - root)
            print(f"stack {k} ray {r} level {lvl}: root {root:.5f}, without the {name} Gaussian it moves by {moved:.2e}, s-tolerance {tol_s:.2e}")
            assert moved >= MARKER_FACTOR * tol_s


@pytest.mark.parametrize("n", [RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1])
def test_wide_stack_markers(oracle, n):
    sc = S.wide_stack(oracle, RAY_LCAP, n)
    o, d = S.wide_rays()
    assert S.kept(o, d, sc.g).all()
    mods = S.models(o, d, sc.g)
    lvl = S.WIDE_MARKER_LEVEL
    assert sorted(sc.markers) == sorted({0, RAY_LCAP - 1, RAY_LCAP, n - 1} & set(range(n)))
    for r, m in mods.items():
        root, tol_s = m.root(lvl), S.s_tolerance(m, lvl, TOL)
        assert root is not None and tol_s is not None and m.root(S.WIDE_MISS_LEVEL) is None
        assert all(m.root(t) is not None for t in S.WIDE_LEVELS)
        for k in sc.markers:
            other = S.RayModel(o, d[r], np.delete(sc.g, k)).root(lvl)
            moved = math.inf if other is None else abs(other - root)
            assert moved >= MARKER_FACTOR * tol_s, (r, k, moved, tol_s)
        print(f"wide stack {n} ray {r}: T_inf {m.T_inf:.3f}, root({lvl}) {root:.4f}, s-tolerance {tol_s:.2e}")


def case_lists(oracle):
    """(name, origins, directions, scene, levels) of every miss check of the GPU suite"""
    g16 = oracle.grid_scene(16)
    out = []
    for name, (o, d) in (("coherent", S.coherent_rays(g16)), ("scattered", S.scattered_rays(g16))):
        out += [(name, o, d, g16, S.PARITY_LEVELS), (name + " per ray", o, d, g16, S.per_ray_levels(S.PARITY_LEVELS, len(d)))]
    at, over = S.one_over_pair(oracle)
    stack_levels = np.concatenate([S.STACK_LEVELS, S.STACK_MARKER_LEVELS, [S.STACK_MISS_LEVEL]]).astype(np.float32)
    o, d = S.stack_rays()
    out += [("stack 31", o, d, S.stack_with_side(oracle, RAY_PL - 1), stack_levels), ("stack 32", o, d, at, stack_levels), ("stack 33", o, d, over, stack_levels)]
    wide_levels = np.concatenate([S.WIDE_LEVELS, [S.WIDE_MARKER_LEVEL, S.WIDE_MISS_LEVEL]]).astype(np.float32)
    o, d = S.wide_rays()
    out += [(f"wide {n}", o, d, S.wide_stack(oracle, RAY_LCAP, n).g, wide_levels) for n in (RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1)]
    return out


def test_the_miss_checks_exclude_at_most_five_percent(oracle):
    """Per case list of the GPU suite: the share of (ray, level) pairs whose T_inf is within tol_T of the level; and both classes occur
    somewhere -- rays that reach a level and rays that do not."""
    seen = set()
    for name, o, d, g, levels in case_lists(oracle):
        for erf_kind in (0, 1):
            cls = S.miss_classes(S.models(o, d, g, erf_kind=erf_kind), levels, S.ray_tolerances(o, d, g))
            share = float((cls == 0).mean())
            print(f"{name}, Erf kind {erf_kind}: {int((cls == 1).sum())} misses, {int((cls == -1).sum())} finite, {int((cls == 0).sum())} excluded ({share:.1%})")
            assert share <= S.EXCLUDED_CAP, name
            assert (cls == 1).any() and (cls == -1).any(), name
            seen |= set(np.unique(cls).tolist())
    assert {1, -1} <= seen


def test_the_side_column_gives_the_wave_mates_depths_of_their_own(oracle):
    """stack_with_side: of the 62 rays aimed 0.6 off the axis some fall below 0.9 behind the side column, most keep nothing."""
    at, over = S.one_over_pair(oracle)
    o, d = S.stack_rays()
    for g in (at, over):
        mods = S.models(o, d, g, rays=range(2, 64))
        lit = [r for r, m in mods.items() if m.T_inf < 0.9 - TOL]
        free = [r for r, m in mods.items() if len(m.w) == 0]
        print(f"wave-mates below 0.9: {lit}; keeping nothing: {len(free)}")
        assert 2 in lit and len(free) >= 40
