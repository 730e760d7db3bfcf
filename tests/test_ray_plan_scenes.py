"""CPU checks of tests/ray_plan_scenes.py with the oracle alone: the plan model restates the bundles' cull, its cases stand on the edges
they claim, each one-line wrong variant of a plan shows on some case, the frozen-list pair is worth what tests/test_gpu_ray_plans.py
holds the GPU to -- and the binding knows the plan's symbols."""
import numpy as np
import pytest

import ray_bundle_scenes as R
import ray_plan_scenes as P
from ray_bundle_scenes import RAY_LCAP, RAY_PL


@pytest.fixture(scope="module")
def scenes(oracle):
    return {sc.name: sc for sc in P.all_scenes(oracle)}


@pytest.fixture(scope="module")
def frozen(oracle):
    return P.frozen_pair(oracle)


def plan_of(sc, **kw):
    return P.model(sc.o, sc.d, sc.g, **kw)


def test_the_model_is_the_cull_in_csr(scenes):
    for sc in scenes.values():
        p = plan_of(sc)
        keep = R.kept(sc.o, sc.d, sc.g)
        assert len(p.offsets) == len(sc.d) + 1 and p.offsets[0] == 0 and p.offsets[-1] == len(p.entries) == keep.sum()
        for r, l in enumerate(p.lists()):
            assert (np.diff(l.astype(np.int64)) > 0).all() and np.array_equal(np.nonzero(keep[r])[0], l), (sc.name, r)
        assert np.array_equal(p.queue, np.nonzero(keep.sum(1) > RAY_PL)[0])
        i, s = p.info(), p.stats()
        assert i["short_rays"] + i["long_rays"] == i["rays"] == s["rays"] == len(sc.d)
        assert (s["short_rays"], s["long_rays"], s["scratch_rays"]) == (i["short_rays"], i["long_rays"], i["scratch_rays"])
        assert s["chunks_tested"] == s["chunks_kept"] == s["members_tested"] == 0


def test_the_cases_stand_on_their_edges(scenes):
    for k in (RAY_PL - 1, RAY_PL, RAY_PL + 1):
        p = plan_of(scenes[f"stack {k}"])
        assert list(p.lens[:2]) == [k, k] and p.info()["long_rays"] == (2 if k > RAY_PL else 0)     # the two axial rays alone keep the stack
        assert (p.lens[2:] <= 5).all() and (p.lens[2:] > 0).any() and (p.lens[2:] == 0).any()       # wave-mates with a few, and with nothing
    for n in (RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1):
        p = plan_of(scenes[f"wide {n}"])
        assert list(p.lens) == [n, n, n] and p.info()["scratch_rays"] == (3 if n > RAY_LCAP else 0) and p.info()["longest"] == n
    for n in (63, 64, 65, 129):
        sc = scenes[f"ragged {n}"]
        assert len(sc.g) == n and plan_of(sc).lens[0] == n - 5 and R.kept(sc.o, sc.d, sc.g)[:, n - 1].any()    # the last chunk's last Gaussian is kept
    assert plan_of(scenes["empty"]).info() == {"rays": 5, "entries": 0, "short_rays": 5, "long_rays": 0, "longest": 0, "scratch_rays": 0}
    for kind in ("scattered", "coherent"):
        sc = scenes[f"grid16 {kind}"]
        lo, hi = R.kept_range(sc.o, sc.d, sc.g)
        assert len(sc.d) == 130 and (lo == hi).all()                                               # every decision is float32's too
        i = plan_of(sc).info()
        assert i["short_rays"] > 0 and (i["long_rays"] > 0 or kind == "coherent")                  # the scattered bundle runs both kernels


def test_every_wrong_plan_shows_on_some_case(scenes):
    names = sorted(scenes)
    for variant in P.WRONG:
        seen = []
        for k, name in enumerate(names):
            sc = scenes[name]
            stale = plan_of(scenes[names[(k + 1) % len(names)]])            # the queue of another bundle
            if plan_of(sc, variant=variant, stale=stale).observed() != plan_of(sc).observed():
                seen.append(name)
        print(f"{variant}: shows on {seen}")
        assert seen, variant
    # and where each is expected to bite
    sc = scenes[f"stack {RAY_PL}"]
    assert plan_of(sc, variant="long_ge").stats()["long_rays"] == 2 and plan_of(sc).stats()["long_rays"] == 0
    sc = scenes["grid16 scattered"]
    assert plan_of(sc, variant="morton_order").observed()[0] != plan_of(sc).observed()[0]
    assert sorted(map(sorted, plan_of(sc, variant="slot_order").observed()[0])) == sorted(map(sorted, plan_of(sc).observed()[0]))     # the same lists, at other rays


def test_sizes_take_the_first_rays(scenes):
    sc = scenes["grid16 scattered"]
    full = plan_of(sc)
    for n in P.SIZES:
        part = plan_of(P.first_rays(sc, n))
        assert part.observed()[0] == full.observed()[0][:n]
    per_ray = P.per_ray_origins(scenes[f"stack {RAY_PL + 1}"])
    assert per_ray.o.shape == per_ray.d.shape and plan_of(per_ray).observed() == plan_of(scenes[f"stack {RAY_PL + 1}"]).observed()


def test_the_frozen_pair_moves_markers_in_and_out(frozen):
    fz = frozen
    assert len(fz.A) == len(fz.B) and len(fz.marker_rays) == P.NMARK
    same = np.ones(len(fz.A), bool)
    same[fz.enter] = same[fz.leave] = same[fz.stay] = False
    assert fz.A[same].tobytes() == fz.B[same].tobytes()                                             # the same cloud
    for f in ("albedo", "sigma", "magnitude"):
        assert np.array_equal(fz.A[f], fz.B[f])                                                     # the markers only MOVE
    kA, kB = R.kept(fz.o, fz.d, fz.A), R.kept(fz.o, fz.d, fz.B)
    for i, r in enumerate(fz.marker_rays):
        assert kB[r, fz.enter[i]] and not kA[:, fz.enter[i]].any()                                  # enters the reach of its ray; out of everyone's before
        assert kA[r, fz.leave[i]] and not kB[:, fz.leave[i]].any()                                  # leaves it; out of everyone's afterwards
        assert kA[r, fz.stay[i]] and kB[r, fz.stay[i]]                                              # moves, and its ray keeps it in both
    for g in (fz.A, fz.B):
        lo, hi = R.kept_range(fz.o, fz.d, g)
        assert (lo == hi).all()                                                                     # no decision inside the model's margin
    assert (kA[:, same] == kB[:, same]).all()


def test_the_frozen_lists_are_worth_ten_tolerances_on_every_marker_ray(oracle, frozen):
    dL, dT, tolL, tolT = P.frozen_worth(oracle, frozen)
    for i, r in enumerate(frozen.marker_rays):
        print(f"marker ray {r}: |dL| {dL[i]:.4f} = {dL[i] / tolL[i]:.0f} tol, |dT| {dT[i]:.4f} = {dT[i] / tolT[i]:.0f} tol")
    assert (dL >= P.MARKER_FACTOR * tolL).all() and (dT >= P.MARKER_FACTOR * tolT).all()
    # and the frozen scene is B under A's lists
    sc = frozen.scene("B", frozen=True)
    assert sc.g is frozen.B and all(np.array_equal(a, b) for a, b in zip(sc.lists(), frozen.scene("A").lists()))
    assert any(not np.array_equal(a, b) for a, b in zip(sc.lists(), frozen.scene("B").lists()))


def test_the_binding_has_the_plan(pkg):
    for name in ("vrt_hip_ray_plan_create_device", "vrt_hip_ray_plan_create", "vrt_hip_ray_plan_destroy", "vrt_hip_set_ray_plan",
                 "vrt_hip_get_ray_plan_info", "vrt_hip_get_ray_plan_lists"):
        assert name in pkg.SYMBOLS, name
        assert hasattr(pkg.lib(), name), name
    assert pkg.PLAN_KEEP_LISTS == 1
    for method in ("ray_plan", "ray_plan_device", "set_ray_plan", "using"):
        assert callable(getattr(pkg.Renderer, method)), method
    for method in ("info", "lists", "close"):
        assert callable(getattr(pkg.RayPlan, method)), method
    assert [k for k, _ in pkg.RayPlanInfo._fields_] == ["rays", "entries", "short_rays", "long_rays", "longest", "scratch_rays", "bytes", "sorted",
                                                        "indexed", "scene_n", "cull_generation"]
    import inspect
    from sgrt_amd import autograd
    for fn in (autograd.radiance_rays, autograd.transmittance_bundle, autograd.depth_bundle):
        assert inspect.signature(fn).parameters["plan"].default is None
