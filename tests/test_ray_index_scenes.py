"""The model of the ray bundles' Morton index (tests/ray_index_scenes.py) and its scenes, checked without a GPU: the index's spheres
never hide a Gaussian the cull rule keeps, the shuffled stacks really need their lists put back into scene order, the index cuts the
leaf spheres a ray keeps on `-g 64` to a few, and the library exports the new entry points."""
import ctypes as C

import numpy as np
import pytest

import ray_bundle_scenes as S
import ray_index_scenes as X
from ray_bundle_scenes import RAY_PL, RAY_LCAP, TOL, MARKER_FACTOR


def test_library_exports_the_ray_index_symbols(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    missing = [s for s in ("vrt_hip_set_ray_index", "vrt_hip_get_ray_index_stats") if not hasattr(lib, s)]
    assert not missing, missing
    assert {"vrt_hip_set_ray_index", "vrt_hip_get_ray_index_stats"} <= set(pkg.SYMBOLS)
    fields = [k for k, _ in pkg.RayIndexStats._fields_]
    assert fields == ["indexed", "groups", "leaves", "groups_tested", "groups_kept", "leaves_tested", "leaves_kept", "members_tested"]
    assert C.sizeof(pkg.RayIndexStats) == 64 and C.sizeof(pkg.RayStats) == 72          # the old struct is as it was
    assert hasattr(pkg.Renderer, "set_ray_index") and hasattr(pkg.Renderer, "ray_index_stats")


def test_morton_order_is_a_stable_function_of_the_scene(oracle):
    g = oracle.grid_scene(16)                                       # constant z: that axis quantises to 0
    key = X.morton_keys(g)
    assert (key & 0x24924924).max() == 0 and len(np.unique(key)) == len(g)
    perm = X.morton_order(g)
    assert sorted(perm) == list(range(len(g))) and (np.diff(key[perm].astype(np.int64)) > 0).all()
    twins = np.concatenate([g[:5], g[:5]])                          # equal keys: scene order decides
    assert (X.morton_order(twins).reshape(5, 2) % 5 == np.arange(5)[:, None]).all()
    assert (np.diff(X.morton_order(twins).reshape(5, 2), axis=1) == 5).all()
    bad = g[:8].copy()
    bad["mu"][3, 0] = np.nan
    assert X.morton_keys(bad)[3] == 0 and X.morton_order(bad)[0] in (0, 3)


def test_the_index_covers_the_cull_rule_on_every_gpu_case(oracle):
    for name, (g, o, d, eps) in X.cases(oracle).items():
        for exp_kind in (1, 0):
            idx = X.Index(g, eps, exp_kind)
            assert len(idx.leaves) == -(-len(g) // 64) and len(idx.groups) == -(-len(idx.leaves) // 64)
            tr = X.Traversal(idx, o, d)
            keep = S.kept(o, d, g, eps, exp_kind)
            assert keep.any(), name
            assert tr.covers(keep), (name, exp_kind)
            assert (tr.leaf[0] <= tr.leaf[1]).all() and (tr.leaf[1] <= tr.leaf[2]).all()
    assert len(X.Index(X.cloud(oracle, 8193)).groups) == 3 and len(X.Index(X.cloud(oracle, 8193)).leaves) == 129


@pytest.mark.parametrize("k", [RAY_PL - 1, RAY_PL, RAY_PL + 1])
def test_shuffled_stack_needs_its_list_sorted_back(oracle, k):
    g = X.shuffled_stack_with_side(oracle, k)
    o, d = S.stack_rays()
    lo, hi = S.kept_range(o, d, g)
    assert (lo[:2] == k).all() and (hi[:2] == k).all()              # still exactly k on the axis
    keep = S.kept(o, d, g)
    perm = X.morton_order(g)
    for r in (0, 1):
        arrival = perm[keep[r][perm]]                               # the kept Gaussians in the order the indexed cull meets them
        assert len(arrival) == k and (np.sort(arrival) != arrival).sum() >= k // 2
    assert (keep[2:].sum(1) > 0).sum() >= 3                         # wave-mates with lists of their own


@pytest.mark.parametrize("n", [RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1])
def test_shuffled_wide_stack_keeps_its_markers_in_place(oracle, n):
    sc = X.shuffled_wide_stack(oracle, RAY_LCAP, n)
    plain = S.wide_stack(oracle, RAY_LCAP, n)
    assert sc.markers == plain.markers and (sc.g[sc.markers] == plain.g[plain.markers]).all()
    assert sorted(sc.g.tobytes()[i:i + 40] for i in range(0, 40 * n, 40)) == sorted(plain.g.tobytes()[i:i + 40] for i in range(0, 40 * n, 40))
    o, d = S.wide_rays()
    lo, hi = S.kept_range(o, d, sc.g)
    assert (lo == n).all() and (hi == n).all()
    perm = X.morton_order(sc.g)
    assert (perm != np.arange(n)).sum() >= n // 2                   # the bitmap is what orders this list
    if n == RAY_LCAP + 1:                                           # the markers are seen: each moves the rays by ten tolerances
        full = S.oracle_radiance(oracle, o, d, sc.g)
        for m in sc.markers:
            less = S.oracle_radiance(oracle, o, d, np.delete(sc.g, m))
            assert np.abs(less - full).max(1).min() >= MARKER_FACTOR * TOL * max(1.0, float(full.max())), m


def test_the_index_leaves_a_ray_of_the_large_grid_a_few_leaves(oracle):
    g, o, d, eps = X.cases(oracle)["g64-coherent"]
    assert len(d) == 130
    tr = X.Traversal(X.Index(g, eps), o, d)
    mean = tr.leaf[1].sum() / len(d)
    runs = S.kept(o, d, g)                                          # for comparison: leaves of consecutive runs holding a kept Gaussian
    print(f"-g 64: {mean:.2f} of {len(tr.index.leaves)} Morton leaves kept per ray; {runs.sum(1).mean():.1f} Gaussians kept per ray")
    assert mean <= 4.0
    assert tr.leaves_kept()[1] / len(d) <= 4.0
    # (these rays are aimed at random Gaussians: a WAVE of them visits the union of its lanes' leaves, most of the scene)
    assert 130 * 64 <= tr.members_tested_max() <= 130 * len(g)


def test_clouds_reach_both_kernels_at_the_large_sizes(oracle):
    for n in X.CLOUD_SIZES:
        g = X.cloud(oracle, n)
        o, d = X.cloud_rays(g)
        lo, hi = S.kept_range(o, d, g)
        assert len(d) == 70 and lo.min() >= 1
        if n >= 4095:
            assert (hi <= RAY_PL).sum() >= 5 and (lo > RAY_PL).sum() >= 5, (n, lo, hi)
