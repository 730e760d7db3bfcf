"""The boundary scenes of tests/test_gpu_boundaries.py can see what they are built to see -- a property of the reference alone,
checked with the oracle on the CPU, with the same builder and the same pixels as the GPU tests.

The condition: for every marker k of a scene there is a checked pixel where the oracle's radiance of the scene WITHOUT Gaussian k
differs from the oracle's radiance of the full scene by at least ten times the tolerance the GPU test applies to that scene.  Ten,
because the GPU result may sit a whole tolerance from the oracle in either direction and a lost element must still be unmistakable.
"""
import numpy as np
import pytest

import boundary_scenes as B


def _check_markers(oracle, sc, tol_of_peak):
    effects, peak = B.marker_effects(oracle, sc, threads=8)
    tol = tol_of_peak(peak)
    worst = min(effects.values())
    print(f"n={sc.n} cap={sc.cap} pixels={list(sc.pixels[:4])} peak={peak:.3f} markers={sc.markers} "
          f"smallest marker effect {worst:.3g} against tolerance {tol:.1e} (x{worst / tol:.0f})")
    assert peak > 0.05
    for k, e in effects.items():
        assert e >= B.MARKER_FACTOR * tol, (k, e, tol)


def test_marker_indices_sit_on_the_edges():
    assert B.marker_indices(24, 23) == [0, 22] and B.marker_indices(24, 24) == [0, 23] and B.marker_indices(24, 25) == [0, 23, 24]
    assert B.marker_indices(1024, 1025) == [0, 1023, 1024]
    assert B.marker_indices(64, 65, chunked=True) == [0, 63, 64]
    assert B.marker_indices(128, 129, chunked=True) == [0, 63, 64, 127, 128]
    assert B.marker_indices(128, 127, chunked=True) == [0, 63, 64, 126]
    assert B.marker_indices(8192, 8193, chunked=True) == [0, 63, 64, 8191, 8192]


@pytest.mark.parametrize("name,cap,n,w,h,chunked,compact", B.CLOUD_CASES + B.CHUNK_CASES,
                         ids=[f"{c[0]}-{c[2]}" for c in B.CLOUD_CASES + B.CHUNK_CASES])
def test_cloud_markers_matter_and_every_ray_sees_the_whole_scene(oracle, name, cap, n, w, h, chunked, compact):
    sc = B.cloud(oracle, cap, n, w, h, chunked, compact, npix=2 if n > 2000 else 3)
    assert sc.markers == B.marker_indices(cap, n, chunked) and len(sc.g) == n
    assert B.all_rays_see_all(sc)                           # with cull_eps = 0: every list of every level holds all n
    # the chunk cases are held against TOL * max(1, peak) by their GPU test whatever n (25 and more: the dense path)
    _check_markers(oracle, sc, lambda peak: B.tolerance(n, peak))


@pytest.mark.parametrize("name,cap,n,w,h,chunked,compact", B.CSTRIDE_CASES, ids=[f"cstride-{c[2]}" for c in B.CSTRIDE_CASES])
def test_cstride_markers_matter(oracle, name, cap, n, w, h, chunked, compact):
    sc = B.cloud(oracle, cap, n, w, h, chunked, compact, npix=2)
    assert (w // 32) * (h // 32) > B.MAX_FUSED_CELLS          # a tile the fused list kernel does not take
    _check_markers(oracle, sc, lambda peak: B.tolerance(n, peak))


@pytest.mark.parametrize("cap,n", B.LATTICE_CASES)
def test_lattice_markers_matter_and_no_ray_sees_many(oracle, cap, n):
    sc = B.lattice(oracle, cap, n)
    assert B.visible_per_ray(sc).max() <= B.PL / 2          # far from the hand-over: the CELL's list is what crosses the limit
    _check_markers(oracle, sc, lambda peak: B.TOL)


def test_one_lane_over_scene(oracle):
    sc = B.one_lane_over(oracle)
    # generous and strict bound of what a ray keeps: the cull's threshold lies between cull_eps and cull_eps * 1365 / n
    for eps in (1e-9, 1e-9 * 1365 / sc.n):
        v = B.visible_per_ray(sc, eps)
        assert v[sc.lane_pixel] == B.PL + 1 and (np.delete(v, sc.lane_pixel) == B.PL).all()
    _check_markers(oracle, sc, lambda peak: B.TOL)


@pytest.mark.parametrize("n", [B.PRUNE_PL - 1, B.PRUNE_PL, B.PRUNE_PL + 1])
def test_prunable_scene(oracle, n):
    sc = B.prunable(oracle, n)
    assert (B.visible_per_ray(sc, 1e-9 * 1365 / n) == n).all()              # every ray keeps all n at the ray level's threshold
    faint = B.Scene(sc, g=sc.g[n - sc.faint:])
    assert (B.visible_per_ray(faint, 5e-7) == sc.faint).all()                                          # each faint one carries at least 5e-7 on every ray ...
    assert sc.faint * 1e-6 < 6 * 1365 * 1e-9                                # ... and all of them together fit the prune's budget

