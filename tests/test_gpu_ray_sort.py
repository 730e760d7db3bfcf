"""Sorted ray bundles on the GPU (vrt_hip_set_ray_sort, csrc/vrt_ray_sort_kernel.hip): with the switch on every bundle entry point
gives the SAME words at the same ray index as with it off, bit for bit; the order is the stable sort of the documented keys, as
tests/ray_sort_scenes.py models it; and a bundle whose neighbours share nothing tests at most half the members.  The bundles are that
file's (tests/test_ray_sort_scenes.py shows on the CPU what they can see); every bundle is shaded once with the sort off and once
with it on, and the tests share those results.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import grad_bundle_scenes as G
import ray_sort_scenes as R
import trans_grad_bundle_scenes as T
from conftest import ROOT
from ray_bundle_scenes import RAY_PL, RAY_LCAP

pytestmark = pytest.mark.gpu
SAME_STATS = ("rays", "short_rays", "long_rays", "lane_entries", "lane_pairs", "scratch_rays")
SAME_INDEX_STATS = ("groups_kept", "leaves_kept")
SAMPLES = np.array([3.5, 4.4, 5.0, 5.6, 6.5], np.float32)      # through the cloud and the stacks from z = -4: one more than a walk's four
LEVELS = np.array([0.9, 0.5, 0.1], np.float32)
_bundles, _cache = {}, {}


def bundle(oracle, name):
    """(g, origins, dirs) by name: cloud-<rays>[-origins] (the main case's scene), wide-<cap>-<n>."""
    if name not in _bundles:
        kind, *rest = name.split("-")
        if kind == "cloud":
            g = R.cloud(oracle, R.MAIN_N)
            o, d = R.aimed_rays(g, int(rest[0]), R.MAIN_SEED, per_ray_origin=len(rest) > 1)
            _bundles[name] = (g, o, d)
        else:
            _bundles[name] = R.wide_case(oracle, int(rest[0]), int(rest[1]))
    return _bundles[name]


CLOUDS = [f"cloud-{n}" for n in R.SIZES if n] + ["cloud-130-origins"]
WIDES = [f"wide-{cap}-{n}" for cap, n in R.WIDE]


def inputs(name, nrays):
    rng = np.random.default_rng(len(name) * 1000 + nrays)
    return {"gr": rng.uniform(-1.0, 1.0, size=(nrays, 4)).astype(np.float32),
            "gT": rng.uniform(-1.0, 1.0, size=(nrays, len(SAMPLES))).astype(np.float32),
            "s_ray": (SAMPLES[None, :] + rng.uniform(-0.2, 0.2, size=(nrays, len(SAMPLES)))).astype(np.float32)}


def shade(r, o, d, x):
    """Every field of every bundle entry point for one (bundle, index, sort): a dict of arrays, and the statistics."""
    out = {}
    out["radiance"], out["pixels"] = r.radiance_rays(o, d, want_image=True)
    out["sort_stats"], out["ray_stats"], out["index_stats"] = r.ray_sort_stats(), r.ray_stats(), r.ray_index_stats()
    out["order"] = r.ray_order() if out["sort_stats"]["sorted"] else None
    out["T shared samples"] = r.transmittance_bundle(o, d, SAMPLES)
    out["T samples per ray"] = r.transmittance_bundle(o, d, x["s_ray"])
    out["depth"] = r.depth_bundle(o, d, LEVELS)
    out["sorted every kind"] = [out["sort_stats"]["sorted"], r.ray_sort_stats()["sorted"]]
    table, rows = r.radiance_rays_grad(o, d, x["gr"], want_rays=True)
    out["atomic table"] = G.table_of(table)
    out["grad ray rows origin"], out["grad ray rows dir"] = rows["origin"], rows["dir"]
    ttable, out["grad_s"], trows = r.transmittance_bundle_grad(o, d, x["s_ray"], x["gT"], want_rays=True)
    out["atomic T table"] = T.table_of(ttable)
    out["tgrad ray rows origin"], out["tgrad ray rows dir"] = trows["origin"], trows["dir"]
    r.set_grad_ordered(1)
    try:
        table = r.radiance_rays_grad(o, d, x["gr"])
        out["ordered table"] = G.table_of(table)
        out["records gauss"], out["records ray"], out["records rows"] = r.grad_records()
        out["sorted every kind"].append(r.ray_sort_stats()["sorted"])
        ttable, _ = r.transmittance_bundle_grad(o, d, x["s_ray"], x["gT"])
        out["ordered T table"] = T.table_of(ttable)
        out["T records gauss"], out["T records ray"], out["T records rows"] = r.grad_records()
        out["mismatches"] = r.grad_ordered_stats()["mismatches"]
    finally:
        r.set_grad_ordered(0)
    return out


BITS = ("radiance", "pixels", "T shared samples", "T samples per ray", "depth", "grad ray rows origin", "grad ray rows dir", "grad_s",
        "tgrad ray rows origin", "tgrad ray rows dir", "ordered table", "records gauss", "records ray", "records rows", "ordered T table",
        "T records gauss", "T records ray", "T records rows")


def off_and_on(renderer, oracle, name, indexed):
    """The bundle shaded with the sort off [0] and on [1], once per session."""
    key = (name, indexed)
    if key not in _cache:
        g, o, d = bundle(oracle, name)
        renderer.set_gaussians(g)
        renderer.set_options(1, 1, 1e-9)
        renderer.clear_tiles()
        renderer.enable_stats(True)
        renderer.set_ray_index(indexed)
        x = inputs(name, len(d))
        try:
            res = []
            for on in (0, 1):
                renderer.set_ray_sort(on)
                res.append(shade(renderer, o, d, x))
            _cache[key] = res
        finally:
            renderer.set_ray_sort(0)
            renderer.set_ray_index(0)
            renderer.enable_stats(False)
    return _cache[key]


# ---- 1. every word where the caller's ray order puts it, every bit the same ----
@pytest.mark.parametrize("indexed", [0, 1], ids=["chunks", "index"])
@pytest.mark.parametrize("name", CLOUDS + WIDES)
def test_sort_on_is_sort_off_bit_for_bit(renderer, oracle, name, indexed):
    off, on = off_and_on(renderer, oracle, name, indexed)
    nrays = len(bundle(oracle, name)[2])
    assert off["radiance"].max() > 0 and len(off["radiance"]) == nrays and np.isfinite(off["T shared samples"]).all()   # not a comparison of darkness
    assert (off["T shared samples"] < 1).any() and np.abs(off["grad_s"]).max() > 0 and len(off["records gauss"]) > 0
    for k in BITS:
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    assert on["mismatches"] == 0 and off["mismatches"] == 0
    want_sorted = int(nrays > 64)
    assert off["sorted every kind"] == [0, 0, 0] and on["sorted every kind"] == [want_sorted] * 3
    assert on["sort_stats"]["rays"] == nrays and off["sort_stats"] == {"sorted": 0, "rays": nrays, "rays_without_sphere": 0}
    print(name, indexed, on["sort_stats"], on["ray_stats"], on["index_stats"])
    for k in SAME_STATS:
        assert on["ray_stats"][k] == off["ray_stats"][k], k
    for k in SAME_INDEX_STATS + ("indexed", "groups_tested"):
        assert on["index_stats"][k] == off["index_stats"][k], k
    assert on["ray_stats"]["chunks_kept"] == off["ray_stats"]["chunks_kept"] and on["ray_stats"]["chunks_tested"] == off["ray_stats"]["chunks_tested"]


def test_the_cases_reach_both_kernels_and_the_scratch_slot(renderer, oracle):
    st = off_and_on(renderer, oracle, f"wide-{RAY_PL}-{RAY_PL + 1}", 1)[1]["ray_stats"]
    assert st["long_rays"] >= 60 and st["short_rays"] >= 30            # a sorted short kernel files the queue
    st = off_and_on(renderer, oracle, f"wide-{RAY_LCAP}-{RAY_LCAP + 1}", 1)[1]["ray_stats"]
    assert st["long_rays"] >= 100 and st["scratch_rays"] >= 30
    assert off_and_on(renderer, oracle, f"wide-{RAY_PL}-{RAY_PL - 1}", 1)[1]["ray_stats"]["long_rays"] == 0


def test_nothing_and_one_wave_are_not_sorted(renderer, oracle, pkg):
    g, o, d = bundle(oracle, "cloud-130")
    want = off_and_on(renderer, oracle, "cloud-130", 0)[0]["radiance"]
    renderer.set_gaussians(g)
    renderer.set_options(1, 1, 1e-9)
    renderer.set_ray_sort(1)
    try:
        renderer.radiance_rays(o, d)
        assert renderer.ray_sort_stats()["sorted"] == 1
        assert pkg.lib().vrt_hip_radiance_rays(renderer._h, 0, None, 0, None, None, None, 0) == 0      # a bundle of nothing: nothing happens
        assert renderer.ray_sort_stats() == {"sorted": 1, "rays": 130, "rays_without_sphere": 0}
        for n in (1, 64):
            rad = renderer.radiance_rays(o, d[:n])
            assert renderer.ray_sort_stats() == {"sorted": 0, "rays": n, "rays_without_sphere": 0}
            with pytest.raises(pkg.VrtHipError):
                renderer.ray_order()
            np.testing.assert_array_equal(rad, want[:n])
    finally:
        renderer.set_ray_sort(0)


@pytest.mark.parametrize("name", ["cloud-130", f"wide-{RAY_PL}-{RAY_PL + 1}"])
@pytest.mark.parametrize("indexed", [0, 1], ids=["chunks", "index"])
def test_atomic_tables_agree_as_two_runs_of_one_call_do(renderer, oracle, name, indexed):
    """The float-atomic tables depend on the arrival order of their adds, sorted or not: compared within twice the suites' bound, as
    tests/test_gpu_grad_bundles.py and tests/test_gpu_trans_grad_bundles.py compare two runs of the same call -- never bit for bit."""
    off, on = off_and_on(renderer, oracle, name, indexed)
    g, o, d = bundle(oracle, name)
    x = inputs(name, len(d))
    sc = G.GradScene("sort " + name, g, o, d, x["gr"], [])
    _, Ssum = G.model(sc, "vcl-as")
    assert np.abs(off["atomic table"]).max() > 0
    assert (np.abs(on["atomic table"] - off["atomic table"]) <= 2 * G.bound(Ssum)).all()
    m = T.bundle_tgrad(T.Case("sort " + name, sc, 0, x["s_ray"], x["gT"]), "vcl-as", 1e-9)
    assert np.abs(off["atomic T table"]).max() > 0
    assert (np.abs(on["atomic T table"] - off["atomic T table"]) <= 2 * T.bound(m.S)).all()


# ---- 2. the order ----
@pytest.mark.parametrize("indexed", [0, 1], ids=["chunks", "index"])
@pytest.mark.parametrize("name", ["cloud-65", "cloud-130", "cloud-1024", "cloud-130-origins", f"wide-{RAY_PL}-{RAY_PL + 1}"])
def test_the_order_is_the_stable_sort_of_the_modelled_keys(renderer, oracle, name, indexed):
    g, o, d = bundle(oracle, name)
    order, keys = off_and_on(renderer, oracle, name, indexed)[1]["order"]
    sp = R.Spheres(g, o, d, bool(indexed))
    assert len(order) == len(keys) == len(d)
    assert R.order_faults(order, keys) == []                           # a permutation, keys ascending, ties in ray order, no sphere last
    ok = sp.bracket_ok(keys)
    assert ok.all(), (np.flatnonzero(~ok)[:5], keys[~ok][:5])
    assert (keys == sp.keys()).mean() > 0.95                           # and nearly always the float64 key itself
    if name == "cloud-1024" and indexed:
        assert not np.array_equal(order, np.arange(len(d))) and len(np.unique(keys)) >= 32


def test_a_ray_without_a_sphere_is_counted_and_comes_last(renderer, oracle):
    g, o, d = bundle(oracle, "cloud-130")
    d = d.copy()
    d[[5, 77]] = R.S.normalise([[1.0, 0.0, 0.1], [0.0, 1.0, -0.2]])
    renderer.set_gaussians(g)
    renderer.set_options(1, 1, 1e-9)
    renderer.set_ray_index(1)
    renderer.set_ray_sort(1)
    try:
        rad = renderer.radiance_rays(o, d)
        assert renderer.ray_sort_stats() == {"sorted": 1, "rays": 130, "rays_without_sphere": 2}
        order, keys = renderer.ray_order()
    finally:
        renderer.set_ray_sort(0)
        renderer.set_ray_index(0)
    assert list(order[-2:]) == [5, 77] and list(keys[[5, 77]]) == [R.NONE, R.NONE] and (rad[[5, 77]] == 0).all()
    assert R.order_faults(order, keys) == []


def test_the_order_repeats_and_is_the_device_forms(renderer, oracle):
    import torch
    g, o, d = bundle(oracle, "cloud-1024")
    want = off_and_on(renderer, oracle, "cloud-1024", 1)
    renderer.set_gaussians(g)
    renderer.set_options(1, 1, 1e-9)
    renderer.set_ray_index(1)
    renderer.set_ray_sort(1)
    try:
        renderer.radiance_rays(o, d)
        again = renderer.ray_order()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            t_o, t_d = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o, d))
            out = torch.zeros((len(d), 4), dtype=torch.float32, device="cuda")
            st.synchronize()
            renderer.radiance_rays_device(len(d), t_o.data_ptr(), 0, t_d.data_ptr(), out.data_ptr(), stream=st.cuda_stream)
            device = renderer.ray_order()                              # waits for the bundle
            got = out.cpu().numpy()
    finally:
        renderer.set_ray_sort(0)
        renderer.set_ray_index(0)
    for a, b, c in zip(want[1]["order"], again, device):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(got, want[0]["radiance"])


# ---- 3. the effect ----
@pytest.mark.parametrize("indexed", [1, 0], ids=["index", "chunks"])
def test_sorted_waves_test_the_members_the_model_counts(renderer, oracle, indexed):
    g, o, d = R.main_case(oracle)
    o, d, _ = R.shuffled_rays(o, d)
    renderer.set_gaussians(g)
    renderer.set_options(1, 1, 1e-9)
    renderer.clear_tiles()
    renderer.enable_stats(True)
    renderer.set_ray_index(indexed)
    which = "index_stats" if indexed else "ray_stats"
    try:
        res = []
        for on in (0, 1):
            renderer.set_ray_sort(on)
            rad = renderer.radiance_rays(o, d)
            res.append({"radiance": rad, "ray_stats": renderer.ray_stats(), "index_stats": renderer.ray_index_stats(), "sort": renderer.ray_sort_stats()})
        order, keys = renderer.ray_order()
    finally:
        renderer.set_ray_sort(0)
        renderer.set_ray_index(0)
        renderer.enable_stats(False)
    off, on = res
    sp = R.Spheres(g, o, d, bool(indexed))
    lo, hi = sp.members_tested(order, 0), sp.members_tested(order, 2)
    got, unsorted = on[which]["members_tested"], off[which]["members_tested"]
    print("index" if indexed else "chunks", "members tested: unsorted", unsorted, "sorted", got, "model", lo, hi, "ratio", got / unsorted)
    assert on["sort"] == {"sorted": 1, "rays": R.MAIN_RAYS, "rays_without_sphere": 0} and off["sort"]["sorted"] == 0
    np.testing.assert_array_equal(on["radiance"], off["radiance"])
    assert R.order_faults(order, keys) == [] and sp.bracket_ok(keys).all()
    assert lo <= got <= hi
    ident = np.arange(len(d))
    assert sp.members_tested(ident, 0) <= unsorted <= sp.members_tested(ident, 2)
    if indexed:
        assert 2 * got <= unsorted          # tests/test_ray_sort_scenes.py's condition, read from the device
    for k in SAME_STATS:
        assert on["ray_stats"][k] == off["ray_stats"][k], k
    for k in SAME_INDEX_STATS:
        assert on["index_stats"][k] == off["index_stats"][k], k


# ---- 4. state ----
CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import oracle
import ray_sort_scenes as R
from conftest import load_pkg
g, o, d = R.main_case(oracle, 130)
r = load_pkg().Renderer(0)
r.set_gaussians(g)
rad = r.radiance_rays(o, d)
print("sorted", r.ray_sort_stats()["sorted"], rad.tobytes().hex())
r.close()
"""


def test_environment_turns_the_sort_on_at_creation(renderer, oracle):
    want = off_and_on(renderer, oracle, "cloud-130", 0)[0]["radiance"]
    env = dict(os.environ, VRT_HIP_RAY_SORT="1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    word, flag, bits = p.stdout.strip().splitlines()[-1].split()
    assert (word, flag) == ("sorted", "1")
    assert bytes.fromhex(bits) == want.tobytes()


def test_copy_state_carries_the_switch(oracle, pkg):
    g, o, d = bundle(oracle, "cloud-130")
    src, dst = pkg.Renderer(0), pkg.Renderer(0)
    try:
        src.set_gaussians(g)
        want = src.radiance_rays(o, d)
        gen = pkg.lib().vrt_hip_state_generation(src._h)
        src.set_ray_sort(1)
        assert pkg.lib().vrt_hip_state_generation(src._h) > gen         # a state change: holders of mirrors see it
        assert pkg.lib().vrt_hip_copy_state(dst._h, src._h) == 0
        got = dst.radiance_rays(o, d)
        assert dst.ray_sort_stats()["sorted"] == 1
        src.radiance_rays(o, d)
        for a, b in zip(src.ray_order(), dst.ray_order()):
            np.testing.assert_array_equal(a, b)
    finally:
        src.close()
        dst.close()
    np.testing.assert_array_equal(got, want)


def test_switching_off_and_smaller_bundles_and_another_scene_keep_the_bits(renderer, oracle, pkg):
    g, o, d = bundle(oracle, "cloud-1024")
    want = off_and_on(renderer, oracle, "cloud-1024", 1)[0]["radiance"]
    small = oracle.gaussians(*[a[:33] for a in (g["albedo"], g["mu"][:, :3], g["sigma"], g["magnitude"])])
    renderer.set_gaussians(small)
    renderer.set_options(1, 1, 1e-9)
    want_small = renderer.radiance_rays(o, d[:130])
    renderer.set_gaussians(g)
    renderer.set_ray_index(1)
    renderer.set_ray_sort(1)
    try:
        np.testing.assert_array_equal(renderer.radiance_rays(o, d), want)
        np.testing.assert_array_equal(renderer.radiance_rays(o, d[:130]), want[:130])          # a smaller bundle in the larger buffers
        order, keys = renderer.ray_order()
        assert len(order) == 130 and R.order_faults(order, keys) == []
        renderer.set_gaussians(small)                                                            # 33 Gaussians: one leaf, one group
        np.testing.assert_array_equal(renderer.radiance_rays(o, d[:130]), want_small)
        assert renderer.ray_sort_stats()["sorted"] == 1
        renderer.set_ray_sort(0)
        n = C.c_size_t()
        buf = np.zeros(1024, np.uint32)
        u32p = C.POINTER(C.c_uint32)
        assert pkg.lib().vrt_hip_get_ray_order(renderer._h, buf.ctypes.data_as(u32p), None, buf.size, C.byref(n)) == -1      # VRT_HIP_ERR_INVALID
        with pytest.raises(pkg.VrtHipError):
            renderer.ray_order()
        np.testing.assert_array_equal(renderer.radiance_rays(o, d[:130]), want_small)
        assert renderer.ray_sort_stats() == {"sorted": 0, "rays": 130, "rays_without_sphere": 0}
    finally:
        renderer.set_ray_sort(0)
        renderer.set_ray_index(0)
