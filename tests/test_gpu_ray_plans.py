"""Ray plans on the GPU (vrt_hip_ray_plan_create*, vrt_hip_set_ray_plan, csrc/vrt_ray_plan_kernel.hip and the RAY_LIST_PLAN instantiations
of the seven bundle units): a planned call gives the bits of the unplanned call in every kind and form, its lists are the model's of
tests/ray_plan_scenes.py entry for entry, it runs no test of the cull, a strict plan refuses a changed scene, and with KEEP_LISTS the
lists stay in force on another scene -- the function the gradient and tangent bundles differentiate.  tests/test_ray_plan_scenes.py
holds model, cases and the frozen-list pair to account on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grad_bundle_scenes as G
import grad_ordered_scenes as GO
import ray_bundle_scenes as R
import ray_plan_scenes as P
import tangent_bundle_scenes as TG
import trans_grad_bundle_scenes as T
from trans_grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL, TGRAD_DEPTH, TGRAD_T

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simd-gaussian-ray-tracing_amd", "bin")

POISON = 0x7FC12345      # a NaN with a payload: any store to it shows
EXTRA = 3                # poisoned rows behind every device output
TAU = np.array([0.9, 0.6, 1.0], np.float32)
EDGE = [f"stack {k}" for k in (RAY_PL - 1, RAY_PL, RAY_PL + 1)] + [f"wide {n}" for n in (RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1)] \
    + [f"ragged {n}" for n in (63, 64, 65, 129)] + ["empty"]
MODELLED = [f"stack {RAY_PL + 1}", "ragged 65", "grid16 scattered"]      # where the atomic tables are held to the bound between two atomic runs


@pytest.fixture(scope="module")
def scenes(oracle):
    return {sc.name: sc for sc in P.all_scenes(oracle)}


@pytest.fixture(autouse=True)
def clean(renderer):
    """Every test starts and ends with no plan bound and the switches off, whatever it did"""
    yield
    renderer.set_ray_plan(None)
    renderer.set_grad_ordered(0)
    renderer.set_ray_index(0)
    renderer.set_ray_sort(0)
    renderer.enable_stats(False)
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)


def setup(renderer, g, eps=1e-9):
    renderer.set_options(*PAIRS["vcl-as"], eps)
    renderer.set_gaussians(g)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- every kind of bundle, host and device form, as one dict of output words ----
class Inputs:
    """What the fourteen calls take besides the rays, seeded per scene; depths: the unplanned depth bundle's result, where depth mode works"""

    def __init__(self, renderer, sc):
        n, nrays = len(sc.g), len(sc.d)
        rng = np.random.default_rng(1300 + sum(map(ord, sc.name)))
        self.s = T.sample_set(sc, 4, False)
        self.gr = sc.gr
        self.gT = rng.uniform(-1, 1, size=(nrays, len(self.s))).astype(np.float32)
        self.gD = rng.uniform(-1, 1, size=(nrays, len(TAU))).astype(np.float32)
        self.v = TG.packed(rng.uniform(-1, 1, size=(n, 9)).astype(np.float32), n)
        self.rv = TG.packed_rays(rng.uniform(-1, 1, size=(nrays, 6)).astype(np.float32), nrays)
        self.sd = rng.uniform(-1, 1, size=(nrays, len(self.s))).astype(np.float32)
        self.dd = rng.uniform(-1, 1, size=(nrays, len(TAU))).astype(np.float32)
        self.depths = renderer.depth_bundle(sc.o, sc.d, TAU)


def flat(table):
    """A gradient table's dict as [N, 9] float32"""
    return np.concatenate([table["albedo"], table["mu"], table["sigma"][:, None], table["magnitude"][:, None]], 1).astype(np.float32)


def host_all(renderer, sc, x):
    o, d = sc.o, sc.d
    out = {}
    out["radiance"], out["image"] = renderer.radiance_rays(o, d, want_image=True)
    out["T"] = renderer.transmittance_bundle(o, d, x.s)
    out["depth"] = renderer.depth_bundle(o, d, TAU)
    table, rows = renderer.radiance_rays_grad(o, d, x.gr, want_table=True, want_rays=True)
    out["grad table"], out["grad rows"] = flat(table), np.concatenate([rows["origin"], rows["dir"]], 1)
    for mode, s, g, wrt in (("T", x.s, x.gT, TGRAD_T), ("depth", x.depths, x.gD, TGRAD_DEPTH)):
        table, gs, rows = renderer.transmittance_bundle_grad(o, d, s, g, wrt=wrt, s_per_ray=s.ndim == 2, want_rays=True)
        out[f"tgrad {mode} table"], out[f"tgrad {mode} grad_s"] = flat(table), gs
        out[f"tgrad {mode} rows"] = np.concatenate([rows["origin"], rows["dir"]], 1)
    out["tangent"] = renderer.radiance_rays_tangent(o, d, tangent=x.v, ray_tangent=x.rv)
    out["ttangent T"] = renderer.transmittance_bundle_tangent(o, d, x.s, tangent=x.v, ray_tangent=x.rv, s_tangent=x.sd, wrt=TGRAD_T)
    out["ttangent depth"] = renderer.transmittance_bundle_tangent(o, d, x.depths, tangent=x.v, ray_tangent=x.rv, s_tangent=x.dd, wrt=TGRAD_DEPTH, s_per_ray=True)
    return {k: (v if v.dtype == np.uint32 else bits(v)) for k, v in out.items()}


def device_all(renderer, sc, x, stream=None):
    """The device forms over torch tensors; outputs that the kernels store are poisoned first with EXTRA rows to spare, tables start at 0"""
    import torch
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    n, nrays, per_ray = len(sc.g), len(sc.d), sc.o.size != 3
    t_o, t_d = cuda(sc.o), cuda(sc.d)
    po, pd = t_o.data_ptr(), t_d.data_ptr()
    st = 0 if stream is None else stream.cuda_stream
    kept, out = [t_o, t_d], {}

    def poisoned(name, shape):
        t = torch.from_numpy(np.full((shape[0] + EXTRA,) + tuple(shape[1:]), POISON, np.uint32).view(np.float32)).cuda()
        out[name] = t
        return t.data_ptr()

    def table(name):
        t = torch.zeros((max(n, 1), 12), dtype=torch.float32, device="cuda")
        out[name] = t
        return t.data_ptr() if n else 0

    def dev(a):
        kept.append(cuda(a))
        return kept[-1].data_ptr()
    ns, nt = len(x.s), len(TAU)
    torch.cuda.synchronize()
    renderer.radiance_rays_device(nrays, po, per_ray, pd, d_radiance=poisoned("radiance", (nrays, 4)), d_image=poisoned("image", (nrays,)), stream=st)
    renderer.transmittance_bundle_device(nrays, po, per_ray, pd, dev(x.s), ns, False, poisoned("T", (nrays, ns)), stream=st)
    renderer.depth_bundle_device(nrays, po, per_ray, pd, dev(TAU), nt, False, poisoned("depth", (nrays, nt)), stream=st)
    if n:
        renderer.radiance_rays_grad_rays_device(nrays, po, per_ray, pd, dev(x.gr), d_grad=table("grad table"), d_grad_rays=poisoned("grad rows", (nrays, 8)),
                                                stream=st)
        for mode, s, g, wrt in (("T", x.s, x.gT, TGRAD_T), ("depth", x.depths, x.gD, TGRAD_DEPTH)):
            renderer.transmittance_bundle_grad_rays_device(nrays, po, per_ray, pd, dev(s), s.shape[-1], s.ndim == 2, dev(g), wrt,
                                                           d_grad=table(f"tgrad {mode} table"), d_grad_s=poisoned(f"tgrad {mode} grad_s", g.shape),
                                                           d_grad_rays=poisoned(f"tgrad {mode} rows", (nrays, 8)), stream=st)
        renderer.radiance_rays_tangent_device(nrays, po, per_ray, pd, d_tangent=dev(x.v), d_ray_tangent=dev(x.rv), d_out=poisoned("tangent", (nrays, 4)), stream=st)
        renderer.transmittance_bundle_tangent_device(nrays, po, per_ray, pd, dev(x.s), ns, False, TGRAD_T, d_tangent=dev(x.v), d_ray_tangent=dev(x.rv),
                                                     d_s_tangent=dev(x.sd), s_tangent_per_ray=True, d_out=poisoned("ttangent T", (nrays, ns)), stream=st)
        renderer.transmittance_bundle_tangent_device(nrays, po, per_ray, pd, dev(x.depths), nt, True, TGRAD_DEPTH, d_tangent=dev(x.v), d_ray_tangent=dev(x.rv),
                                                     d_s_tangent=dev(x.dd), s_tangent_per_ray=True, d_out=poisoned("ttangent depth", (nrays, nt)), stream=st)
    if stream is not None:
        stream.synchronize()
    renderer.sync()
    torch.cuda.synchronize()
    res = {}
    for k, t in out.items():
        a = t.cpu().numpy().view(np.uint32)
        if "table" in k:
            res[k] = a[:n, :9]
        else:
            assert (a[nrays:] == POISON).all(), (sc.name, k)                 # nothing behind the last ray is written
            res[k] = a[:nrays]
    return res


def device_plan(renderer, sc, stream=None):
    import torch
    t_o, t_d = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (sc.o, sc.d))
    torch.cuda.synchronize()
    return renderer.ray_plan_device(len(sc.d), t_o.data_ptr(), sc.o.size != 3, t_d.data_ptr(), stream=0 if stream is None else stream.cuda_stream)


_BOUNDS = {}


def atomic_bounds(sc, x):
    """{output: what two atomic runs of the table may differ by}: twice the model's bound, as the gradient suites hold two runs"""
    if sc.name not in _BOUNDS:
        b = {"grad table": 2 * G.bound(G.bundle_grad(sc, "vcl-as", 1e-9)[1])}
        for mode, s, g, wrt in (("T", x.s, x.gT, TGRAD_T), ("depth", x.depths, x.gD, TGRAD_DEPTH)):
            S = T.bundle_tgrad(T.Case(f"{mode} {sc.name}", sc, wrt, s, g), "vcl-as", 1e-9, s=s).S
            b[f"tgrad {mode} table"] = np.concatenate([np.zeros((len(sc.g), 4)), 2 * T.bound(S)], 1)
        _BOUNDS[sc.name] = b
    return _BOUNDS[sc.name]


def check_same_bits(renderer, sc, forms=("host", "device")):
    setup(renderer, sc.g)
    x = Inputs(renderer, sc)
    for form in forms:
        run = host_all if form == "host" else device_all
        for ordered in (0, 1):
            renderer.set_grad_ordered(ordered)
            want = run(renderer, sc, x)
            plan = renderer.ray_plan(sc.o, sc.d) if form == "host" else device_plan(renderer, sc)
            assert plan.info()["rays"] == len(sc.d) and plan.info()["scene_n"] == len(sc.g)
            with renderer.using(plan):
                got = run(renderer, sc, x)
            plan.close()
            assert sorted(got) == sorted(want)
            for k in want:
                if "table" in k and not ordered:             # float atomics: as two runs differ
                    if sc.name in MODELLED:
                        diff = np.abs(got[k].view(np.float32).astype(np.float64) - want[k].view(np.float32))
                        assert (diff <= atomic_bounds(sc, x)[k]).all(), (sc.name, form, k)
                    continue
                np.testing.assert_array_equal(got[k], want[k], f"{sc.name} {form} ordered {ordered}: {k}")
            assert (want["radiance"] != 0).any() == bool(R.kept(sc.o, sc.d, sc.g).any())


# ---- 1. the same bits, all seven kinds ----
@pytest.mark.parametrize("name", EDGE)
def test_same_bits_on_the_edges(renderer, scenes, name):
    check_same_bits(renderer, scenes[name])


@pytest.mark.parametrize("n", P.SIZES)
def test_same_bits_bundle_sizes_per_ray_origins(renderer, scenes, n):
    check_same_bits(renderer, P.first_rays(scenes["grid16 scattered"], n))


@pytest.mark.parametrize("n", P.SIZES)
def test_same_bits_bundle_sizes_shared_origin(renderer, scenes, n):
    check_same_bits(renderer, P.first_rays(scenes["grid16 coherent"], n), forms=("host",) if n != 130 else ("host", "device"))


def test_same_bits_shared_origin_given_per_ray(renderer, scenes):
    check_same_bits(renderer, P.per_ray_origins(scenes[f"stack {RAY_PL + 1}"]))


def test_a_plan_of_no_rays_and_calls_of_none(renderer, scenes):
    sc = scenes["grid16 scattered"]
    setup(renderer, sc.g)
    plan = renderer.ray_plan(sc.o[:0], sc.d[:0])
    assert plan.info()["rays"] == 0 and plan.info()["entries"] == 0 and list(plan.lists()[0]) == [0]
    with renderer.using(plan):
        assert renderer.radiance_rays(sc.o[:0], sc.d[:0]).shape == (0, 4)
    plan.close()


# ---- 2. the switches ----
def test_lists_are_the_models_under_every_switch(renderer, scenes):
    sc = scenes["grid16 scattered"]
    setup(renderer, sc.g)
    m = P.model(sc.o, sc.d, sc.g)
    want = bits(renderer.radiance_rays(sc.o, sc.d))
    for index in (0, 1):
        for sort in (0, 1):
            renderer.set_ray_index(index)
            renderer.set_ray_sort(sort)
            plan = renderer.ray_plan(sc.o, sc.d)
            offsets, entries = plan.lists()
            np.testing.assert_array_equal(offsets, m.offsets, f"index {index} sort {sort}")
            np.testing.assert_array_equal(entries, m.entries, f"index {index} sort {sort}")
            info = plan.info()
            assert (info["sorted"], info["indexed"]) == (sort, index)
            assert info["bytes"] == 12 * len(sc.d) + 4 * (info["entries"] + info["long_rays"]) + (8 * len(sc.d) if sort else 0)
            assert {k: info[k] for k in m.info()} == m.info()
            if sort:
                renderer.radiance_rays(sc.o, sc.d)
                order, keys = renderer.ray_order()                             # the unplanned sorted call's
                renderer.set_ray_sort(0)                                       # ... and the plan's, whatever the switch says
            with renderer.using(plan):
                for i2 in (0, 1):
                    for s2 in (0, 1):                                          # flipping a switch under a bound strict plan: no bit, not stale
                        renderer.set_ray_index(i2)
                        renderer.set_ray_sort(s2)
                        np.testing.assert_array_equal(bits(renderer.radiance_rays(sc.o, sc.d)), want, f"plan {index} {sort} under {i2} {s2}")
                        assert renderer.ray_sort_stats()["sorted"] == sort
                        if sort:
                            got_order, got_keys = renderer.ray_order()
                            np.testing.assert_array_equal(got_order, order)
                            np.testing.assert_array_equal(got_keys, keys)
            plan.close()


# ---- 3. it really skips the cull ----
@pytest.mark.parametrize("name", ["grid16 scattered", f"wide {RAY_LCAP + 1}", f"stack {RAY_PL + 1}", f"stack {RAY_PL}"])
def test_statistics_of_a_planned_call(renderer, scenes, name):
    sc = scenes[name]
    setup(renderer, sc.g)
    m = P.model(sc.o, sc.d, sc.g)
    renderer.enable_stats(True)
    per_ray = ("rays", "short_rays", "long_rays", "lane_entries", "lane_pairs", "scratch_rays")
    for index in (0, 1):
        renderer.set_ray_index(index)
        renderer.radiance_rays(sc.o, sc.d)
        unplanned = renderer.ray_stats()
        assert renderer.ray_index_stats()["indexed"] == index
        assert (unplanned["members_tested"] if not index else renderer.ray_index_stats()["members_tested"]) > 0
        plan = renderer.ray_plan(sc.o, sc.d)
        assert {k: plan.info()[k] for k in m.info()} == m.info()
        with renderer.using(plan):
            renderer.radiance_rays(sc.o, sc.d)
            planned = renderer.ray_stats()
            assert {k: planned[k] for k in per_ray} == {k: unplanned[k] for k in per_ray}
            assert planned == m.stats()
            assert planned["chunks_tested"] == planned["chunks_kept"] == planned["members_tested"] == 0
            assert set(renderer.ray_index_stats().values()) == {0}
            renderer.set_grad_ordered(1)
            renderer.radiance_rays_grad(sc.o, sc.d, sc.gr)
            st = renderer.grad_ordered_stats()
            assert st["mismatches"] == 0 and st["records"] == GO.record_count(m.lens, True) > 0
            assert renderer.ray_stats() == m.stats()
            renderer.set_grad_ordered(0)
        plan.close()


# ---- 4. strict and stale ----
def raw_calls(renderer, sc):
    """(host(n), device(n), untouched()): vrt_hip_radiance_rays of the first n rays into poisoned outputs, the return codes, and whether
    the outputs still hold nothing but poison"""
    import torch
    L, h = renderer._L, renderer._h
    f32p = C.POINTER(C.c_float)
    o, d = np.ascontiguousarray(sc.o, np.float32), np.ascontiguousarray(sc.d, np.float32)
    out = np.full((len(d), 4), POISON, np.uint32)
    t_o, t_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    t_out = torch.from_numpy(out.copy().view(np.float32)).cuda()
    torch.cuda.synchronize()
    per_ray = int(o.size != 3)

    def host(n):
        return L.vrt_hip_radiance_rays(h, n, o.ctypes.data_as(f32p), per_ray, d.ctypes.data_as(f32p), out.ctypes.data_as(f32p), None, 0)

    def device(n):
        return L.vrt_hip_radiance_rays_device(h, n, t_o.data_ptr(), per_ray, t_d.data_ptr(), t_out.data_ptr(), None, 0, None)

    def untouched():
        renderer.sync()
        torch.cuda.synchronize()
        return bool((out == POISON).all() and (t_out.cpu().numpy().view(np.uint32) == POISON).all())
    return host, device, untouched


def test_a_strict_plan_refuses_a_changed_scene(renderer, scenes, pkg):
    import torch
    sc = scenes[f"stack {RAY_PL + 1}"]
    n = len(sc.d)
    setup(renderer, sc.g)
    want = bits(renderer.radiance_rays(sc.o, sc.d))
    p = G.params64(sc.g)
    t_mu, t_alb, t_sig, t_mag = (torch.tensor(p[k], dtype=torch.float32, device="cuda") for k in ("mu", "albedo", "sigma", "magnitude"))
    torch.cuda.synchronize()
    causes = [(lambda: renderer.set_gaussians(sc.g), b"vrt_hip_set_gaussians)"),
              (lambda: renderer.set_gaussians_device(len(sc.g), t_mu.data_ptr(), t_alb.data_ptr(), t_sig.data_ptr(), t_mag.data_ptr()), b"vrt_hip_set_gaussians_device"),
              (lambda: renderer.set_options(*PAIRS["vcl-as"], 2e-9), b"vrt_hip_set_options")]
    for change, word in causes:
        setup(renderer, sc.g)
        plan = renderer.ray_plan(sc.o, sc.d)
        renderer.set_ray_plan(plan)
        np.testing.assert_array_equal(bits(renderer.radiance_rays(sc.o, sc.d)), want)
        change()
        host, device, untouched = raw_calls(renderer, sc)
        for call in (host, device):
            assert call(n) == -1
            msg = renderer._L.vrt_hip_last_error(renderer._h)
            assert b"stale" in msg and word in msg, msg
        assert untouched()
        with pytest.raises(pkg.VrtHipError):
            renderer.radiance_rays(sc.o, sc.d)
        renderer.set_ray_plan(None)
        assert host(n) == 0 and device(n) == 0 and not untouched()          # the same calls, unplanned
        plan.close()


def test_a_wrong_ray_count_is_refused_and_a_destroyed_plan_is_unbound(renderer, scenes):
    sc = scenes[f"stack {RAY_PL + 1}"]
    n = len(sc.d)
    setup(renderer, sc.g)
    plan = renderer.ray_plan(sc.o, sc.d)
    renderer.set_ray_plan(plan)
    host, device, untouched = raw_calls(renderer, sc)
    for call in (host, device):
        assert call(n - 1) == -1
        msg = renderer._L.vrt_hip_last_error(renderer._h)
        assert str(n).encode() in msg and str(n - 1).encode() in msg, msg
    assert untouched()
    assert host(n) == 0
    plan.close()                                                             # destroying the bound plan unbinds it
    assert renderer._plan == (None, False)
    assert host(n - 1) == 0 and device(n - 1) == 0
    other = renderer.ray_plan(sc.o, sc.d[:5])
    with pytest.raises(Exception):
        renderer.set_ray_plan(plan)                                          # a closed plan has no handle
    assert renderer._L.vrt_hip_set_ray_plan(renderer._h, other._p, 2) == -1  # flags
    other.close()


def test_a_plan_made_on_one_stream_is_used_on_another(renderer, scenes):
    import torch
    sc = scenes["grid16 scattered"]
    setup(renderer, sc.g)
    x = Inputs(renderer, sc)
    want = device_all(renderer, sc, x)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    plan = device_plan(renderer, sc, stream=s1)                              # complete when it returns
    with renderer.using(plan):
        got = device_all(renderer, sc, x, stream=s2)                         # no sync in between
    plan.close()
    for k in want:
        if "table" not in k:
            np.testing.assert_array_equal(got[k], want[k], k)


# ---- 5. frozen lists ----
@pytest.fixture(scope="module")
def frozen(oracle):
    fz = P.frozen_pair(oracle)
    return fz, P.frozen_worth(oracle, fz), P.frozen_tolerances(oracle, fz)


def test_frozen_lists_give_the_sum_over_the_plans_lists(renderer, oracle, frozen):
    fz, (dL, dT, _, _), (tolL, tolT) = frozen
    rays = range(len(fz.d))
    setup(renderer, fz.A)
    plan = renderer.ray_plan(fz.o, fz.d)
    la = fz.scene("A").lists()
    offsets, entries = plan.lists()
    assert [tuple(entries[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])] == [tuple(l) for l in la]
    renderer.set_gaussians(fz.B)
    own_L, own_T = renderer.radiance_rays(fz.o, fz.d), renderer.transmittance_bundle(fz.o, fz.d, P.FROZEN_S)
    with renderer.using(plan, keep_lists=True):
        got_L, got_T = renderer.radiance_rays(fz.o, fz.d), renderer.transmittance_bundle(fz.o, fz.d, P.FROZEN_S)
    want_L = P.list_radiance(oracle, fz.o, fz.d, fz.B, la, rays)
    want_T = P.list_T(oracle, fz.o, fz.d, P.FROZEN_S, fz.B, la, rays)
    eL, eT = np.abs(got_L.astype(np.float64) - want_L).max(1), np.abs(got_T.astype(np.float64) - want_T).max(1)
    print(f"frozen: worst |L - oracle over the plan's lists| / tol {np.max(eL / tolL):.3f}, of T {np.max(eT / tolT):.3f}")
    assert (eL <= tolL).all() and (eT <= tolT).all()
    m = fz.marker_rays
    assert (np.abs(got_L[m].astype(np.float64) - own_L[m]).max(1) > 0.5 * dL).all()
    assert (np.abs(got_T[m].astype(np.float64) - own_T[m]).max(1) > 0.5 * dT).all()
    # strict, the same plan refuses B
    renderer.set_ray_plan(plan)
    with pytest.raises(Exception, match="stale"):
        renderer.radiance_rays(fz.o, fz.d)
    # another N is refused under KEEP_LISTS too
    renderer.set_ray_plan(plan, keep_lists=True)
    renderer.set_gaussians(fz.B[:-1])
    with pytest.raises(Exception, match=f"{len(fz.A)} Gaussians"):
        renderer.radiance_rays(fz.o, fz.d)
    renderer.set_ray_plan(None)
    plan.close()


def test_frozen_tangent_and_gradient_are_adjoint(renderer, oracle, frozen):
    """v = B - A: sum_r u_r . (J v)_r by the planned tangent bundle and <table, v> by the planned gradient bundle, both on B under A's
    lists, within the bound of test_gpu_tangent_bundles.test_adjoint_of_the_gradient_bundle"""
    fz = frozen[0]
    sc = fz.scene("B", frozen=True)
    setup(renderer, fz.A)
    plan = renderer.ray_plan(fz.o, fz.d)
    renderer.set_gaussians(fz.B)
    pa, pb = G.params64(fz.A), G.params64(fz.B)
    v = np.concatenate([pb["albedo"] - pa["albedo"], pb["mu"] - pa["mu"], (pb["sigma"] - pa["sigma"])[:, None], (pb["magnitude"] - pa["magnitude"])[:, None]], 1)
    v = v.astype(np.float32)
    assert np.abs(v[fz.enter]).max() > 1 and np.abs(v[fz.leave]).max() > 1 and 0 < np.abs(v[fz.stay]).max() < 0.1
    assert np.count_nonzero(np.abs(v).max(1)) == 3 * P.NMARK
    u = sc.gr.astype(np.float64)
    with renderer.using(plan, keep_lists=True):
        table = G.table_of(renderer.radiance_rays_grad(fz.o, fz.d, sc.gr))
        Jv = renderer.radiance_rays_tangent(fz.o, fz.d, tangent=TG.packed(v, len(fz.B))).astype(np.float64)
    plan.close()
    St = G.bundle_grad(sc, "vcl-as", 1e-9)[1]
    _, S_T = TG.model(sc, "vcl-as", 1e-9, v[None], np.zeros((1, len(fz.d), 6)))
    v64 = v.astype(np.float64)
    lhs, rhs = (u * Jv).sum(), (table * v64).sum()
    B = (np.abs(u) * TG.bound(S_T[0])).sum() + (G.bound(St) * np.abs(v64)).sum()
    print(f"frozen adjoint: lhs {lhs:.9e} rhs {rhs:.9e} |diff| / B {abs(lhs - rhs) / B:.3f}")
    assert abs(lhs) > 100 * B and abs(lhs - rhs) <= B                        # the markers that stay carry it: far from 0 = 0
    assert (table[fz.enter] == 0).all() and (np.abs(table[fz.stay]).max(1) > 0).all()     # nothing new is picked up


# ---- 6. torch ----
def tensors(g, requires_grad=False):
    import torch
    p = G.params64(g)
    return [torch.tensor(p[k], dtype=torch.float32, device="cuda", requires_grad=requires_grad) for k in ("mu", "albedo", "sigma", "magnitude")]


def test_torch_forward_backward_and_jvp_with_a_plan(renderer, scenes):
    import torch
    from sgrt_amd import autograd
    sc = scenes["grid16 scattered"]
    setup(renderer, sc.g)
    renderer.set_grad_ordered(1)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()      # noqa: E731
    t_o, t_d, t_g = cuda(sc.o), cuda(sc.d), cuda(sc.gr)
    plan = renderer.ray_plan(sc.o, sc.d)
    other = renderer.ray_plan(sc.o, sc.d)
    rng = np.random.default_rng(8)
    tang = [cuda(rng.uniform(-1, 1, size=tuple(t.shape))) for t in tensors(sc.g)]
    results = {}
    for name, p, bound in (("none", None, None), ("plan", plan, None), ("plan under another binding", plan, other)):
        renderer.set_ray_plan(bound, keep_lists=bound is not None)
        before = renderer._plan
        ps = tensors(sc.g, requires_grad=True)
        o = t_o.clone().requires_grad_(True)
        L = autograd.radiance_rays(renderer, *ps, o, t_d, plan=p)
        assert renderer._plan == before
        (L * t_g).sum().backward()
        assert renderer._plan == before
        _, Jv = torch.func.jvp(lambda *a: autograd.radiance_rays(renderer, *a, t_o, t_d, plan=p), tuple(tensors(sc.g)), tuple(tang))
        assert renderer._plan == before
        results[name] = [bits(t.detach().cpu().numpy()) for t in (L, *[q.grad for q in ps], o.grad, Jv)]
        assert all((r != 0).any() for r in results[name])
    renderer.set_ray_plan(None)
    for name in ("plan", "plan under another binding"):
        for a, b in zip(results[name], results["none"]):
            np.testing.assert_array_equal(a, b, name)
    # the profiles take the plan too
    s = cuda(T.sample_set(sc, 3, False))
    for fn, vals in ((autograd.transmittance_bundle, s), (autograd.depth_bundle, cuda(TAU[:2]))):
        outs = []
        for p in (None, plan):
            ps = tensors(sc.g, requires_grad=True)
            out = fn(renderer, *ps, t_o, t_d, vals, plan=p)
            torch.where(torch.isfinite(out), out, torch.zeros_like(out)).sum().backward()
            outs.append([bits(t.detach().cpu().numpy()) for t in (out, ps[0].grad, ps[2].grad, ps[3].grad)])
            assert renderer._plan == (None, False)
        for a, b in zip(*outs):
            np.testing.assert_array_equal(a, b)
    plan.close()
    other.close()


# ---- 7. the C++ example ----
def test_cpp_ray_plan_example(tmp_path):
    """host/ray_plan_example.cpp (vrt::ray_plan, vrt::set_ray_plan, vrt::ray_plan_lists): one plan, three rounds of tangent plus gradient
    bundle on it; the first round has the unplanned bits, and every round's |J v|^2 is its <v, J^T J v>."""
    p = subprocess.run([os.path.join(BIN, "ray_plan_example"), "3"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "planned against unplanned: identical" in p.stderr.splitlines()
    lines = p.stdout.strip().splitlines()
    head = re.fullmatch(r"plan: 256 rays, (\d+) entries, (\d+) short, (\d+) long, longest list (\d+), (\d+) bytes, sorted 0, indexed 0", lines[0])
    assert head and int(head.group(2)) + int(head.group(3)) == 256 and 0 < int(head.group(4)) <= 3, lines[0]
    rounds = [re.fullmatch(r"round (\d): \|J v\|\^2 ([-+0-9.e]+)  <v, J\^T J v> ([-+0-9.e]+)", ln) for ln in lines[1:]]
    assert len(rounds) == 3 and all(rounds), p.stdout
    for m in rounds:        # the example's own sanity line, to a per cent; test_frozen_tangent_and_gradient_are_adjoint holds the identity to the suites' bound
        a, b = float(m.group(2)), float(m.group(3))
        assert a > 0 and abs(a - b) <= 1e-2 * a, (a, b)
