"""The ray-bundle scenes (tests/ray_bundle_scenes.py) test what they claim -- shown with the oracle alone, no GPU: the cull
rule restated in float64 gives the intended list lengths on both sides of RAY_PL and RAY_LCAP, leaving out a marker Gaussian
moves a checked ray by at least ten tolerances, and what the rule drops changes a ray by less than the documented bound."""
import numpy as np
import pytest

import ray_bundle_scenes as S
from ray_bundle_scenes import RAY_PL, RAY_LCAP, TOL, MARKER_FACTOR, CULL_BOUND


def subset_radiance(oracle, o, d, g, keep):
    o = np.asarray(o, np.float32).reshape(-1, 3)
    return np.stack([oracle.radiance(o[r if len(o) > 1 else 0], d[r], g[keep[r]], 1, 1) for r in range(len(d))])


@pytest.mark.parametrize("dim, lo, hi", [(16, 6, 53), (32, 6, 89)])
def test_scattered_rays_run_both_kernels(oracle, dim, lo, hi):
    g = oracle.grid_scene(dim)
    o, d = S.scattered_rays(g)
    keep = S.kept(o, d, g)
    counts = keep.sum(1)
    assert (counts.min(), counts.max()) == (lo, hi)
    assert (counts <= RAY_PL).sum() >= 8 and (counts > RAY_PL).sum() >= 4          # both kernels have rays
    klo, khi = S.kept_range(o, d, g)
    assert (klo <= counts).all() and (counts <= khi).all() and ((khi <= RAY_PL) | (klo > RAY_PL)).sum() >= len(d) - 2
    full = S.oracle_radiance(oracle, o, d, g)
    assert full.max() > 0.05
    dev = np.abs(subset_radiance(oracle, o, d, g, keep).astype(np.float64) - full).max()
    assert dev < CULL_BOUND, dev


def test_coherent_rays_hit_the_grid(oracle):
    g = oracle.grid_scene(16)
    o, d = S.coherent_rays(g)
    assert len(d) == 130                                   # three waves, the last one ragged
    keep = S.kept(o, d, g)
    assert keep.sum(1).min() >= 3 and keep.sum(1).max() <= RAY_PL
    counts0 = S.kept(o, d, g, cull_eps=0.0).sum(1)         # with the cull off the same rays reach both kernels
    assert (counts0 <= RAY_PL).sum() >= 20 and (counts0 > RAY_PL).sum() >= 20
    full = S.oracle_radiance(oracle, o, d, g)
    assert full.max() > 0.05
    assert np.abs(subset_radiance(oracle, o, d, g, keep).astype(np.float64) - full).max() < CULL_BOUND


def test_centre_rays_of_the_large_grid_keep_short_lists(oracle):
    g = oracle.grid_scene(64)
    o, d = S.centre_rays(g)
    counts = S.kept(o, d, g).sum(1)
    assert len(d) == 64 and counts.min() >= 1 and counts.max() <= 10      # n^2 <= 100 pairs against 4096^2


@pytest.mark.parametrize("k", [RAY_PL - 1, RAY_PL, RAY_PL + 1])
def test_stack_sits_on_the_list_capacity(oracle, k):
    g = S.stack(oracle, k)
    o, d = S.stack_rays()
    lo, hi = S.kept_range(o, d, g)
    assert (lo[:2] == k).all() and (hi[:2] == k).all()     # the axial and the near-axial ray keep exactly k ...
    assert (hi[2:] == 0).all() and len(d) == 64            # ... and the 62 others nothing
    full = S.oracle_radiance(oracle, o, d, g, rays=[0, 1])
    less = S.oracle_radiance(oracle, o, d, g[:-1], rays=[0, 1])
    assert np.abs(full - less).max(1).min() >= MARKER_FACTOR * TOL       # the LAST Gaussian of the list is seen
    assert np.abs(S.oracle_radiance(oracle, o, d, g, rays=[2, 33])).max() < 1e-12   # what the misses lose is nothing


@pytest.mark.parametrize("n", [RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1])
def test_wide_stack_sits_on_the_lds_capacity(oracle, n):
    sc = S.wide_stack(oracle, RAY_LCAP, n)
    o, d = S.wide_rays()
    lo, hi = S.kept_range(o, d, sc.g)
    assert (lo == n).all() and (hi == n).all()
    assert sc.markers == sorted({0, RAY_LCAP - 1, RAY_LCAP, n - 1} & set(range(n)))
    full = S.oracle_radiance(oracle, o, d, sc.g)
    for m in sc.markers:
        less = S.oracle_radiance(oracle, o, d, np.delete(sc.g, m))
        assert np.abs(less - full).max(1).min() >= MARKER_FACTOR * TOL * max(1.0, float(full.max())), m


def test_one_over_pair_differs_only_where_the_axial_rays_look(oracle):
    at, over = S.one_over_pair(oracle)
    o, d = S.stack_rays()
    assert len(over) == len(at) + 1 and (np.delete(over, RAY_PL) == at).all()
    k_at, k_over = S.kept(o, d, at), S.kept(o, d, over)
    assert (k_at[:2].sum(1) == RAY_PL).all() and (k_over[:2].sum(1) == RAY_PL + 1).all()
    assert not k_over[2:, :RAY_PL + 1].any()                     # no wave-mate sees the stack, the extra Gaussian included
    assert (np.delete(k_over, RAY_PL, axis=1)[2:] == k_at[2:]).all()
    lit = np.flatnonzero(k_at[2:].sum(1) > 0) + 2
    assert lit.size >= 3                                         # some wave-mates have lists of their own ...
    assert S.oracle_radiance(oracle, o, d, at, rays=lit).max() > 0.05   # ... and light
