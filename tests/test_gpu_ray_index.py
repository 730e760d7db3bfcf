"""The ray bundles' Morton index on the GPU (vrt_hip_set_ray_index, the INDEXED kernels of csrc/vrt_ray_kernel.hip): with the index on
a bundle gives the SAME radiance and the same packed pixels as with it off, bit for bit, sends the same rays to the same kernel, and
really goes through the index, as tests/ray_index_scenes.py models it.  The scenes are that file's (tests/test_ray_index_scenes.py
shows on the CPU that they exercise the sort-back, the bitmap and every size edge); every bundle is shaded once with the index off and
once with it on, and the tests share those results.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ray_bundle_scenes as S
import ray_index_scenes as X
from conftest import ROOT
from ray_bundle_scenes import RAY_PL, RAY_LCAP

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "simd-gaussian-ray-tracing_amd", "bin")
PAIRS = {"vcl-as": (1, 1), "libm-libm": (0, 0)}     # (Exp, Erf): the same numbers in the package and in the oracle
SAME_STATS = ("rays", "short_rays", "long_rays", "lane_entries", "lane_pairs", "scratch_rays")
_cache = {}


def names():
    fixed = ["g16-coherent", "g16-coherent-nocull", "g32-scattered", "g64-centre", "g64-coherent"]
    return (fixed + [f"stack-{k}" for k in (RAY_PL - 1, RAY_PL, RAY_PL + 1)] + [f"wide-{n}" for n in (RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1)]
            + [f"cloud-{n}" for n in X.CLOUD_SIZES])


def shade(r, o, d, on):
    """(radiance, pixels, ray_stats, ray_index_stats) of one bundle; stats are on."""
    r.set_ray_index(on)
    rad, img = r.radiance_rays(o, d, want_image=True)
    return rad, img, r.ray_stats(), r.ray_index_stats()


def off_and_on(renderer, oracle, name, pair="vcl-as"):
    """The case shaded with the index off [0] and on [1], once per session."""
    key = (name, pair)
    if key not in _cache:
        g, o, d, eps = X.cases(oracle)[name]
        renderer.set_gaussians(g)
        renderer.set_options(PAIRS[pair][0], PAIRS[pair][1], eps)
        renderer.clear_tiles()
        renderer.enable_stats(True)
        try:
            _cache[key] = [shade(renderer, o, d, on) for on in (0, 1)]
        finally:
            renderer.set_ray_index(0)
            renderer.enable_stats(False)
    return _cache[key]


# ---- 1. identity, and the same rays in the same kernels ----
@pytest.mark.parametrize("name, pair", [(n, "vcl-as") for n in names()] + [("g16-coherent", "libm-libm"), ("g32-scattered", "libm-libm"),
                                                                            ("stack-33", "libm-libm"), ("cloud-4097", "libm-libm")])
def test_index_on_is_index_off_bit_for_bit(renderer, oracle, name, pair):
    off, on = off_and_on(renderer, oracle, name, pair)
    assert off[0].max() > 0 and len(off[0]) == len(X.cases(oracle)[name][2])        # not a comparison of darkness
    np.testing.assert_array_equal(on[0], off[0])
    np.testing.assert_array_equal(on[1], off[1])
    print(name, pair, off[2], on[3])
    for k in SAME_STATS:
        assert on[2][k] == off[2][k], k
    assert off[3]["indexed"] == 0 and on[3]["indexed"] == 1


def test_the_cases_reach_both_kernels_and_the_scratch_slot(renderer, oracle):
    assert off_and_on(renderer, oracle, "g16-coherent")[0][2]["rays"] == 130
    st = off_and_on(renderer, oracle, "g32-scattered")[1][2]
    assert st["long_rays"] >= 4 and st["short_rays"] >= 8
    for k, n_long in ((RAY_PL - 1, 0), (RAY_PL, 0), (RAY_PL + 1, 2)):
        assert off_and_on(renderer, oracle, f"stack-{k}")[1][2]["long_rays"] == n_long
    for n, scratch in ((RAY_LCAP - 1, 0), (RAY_LCAP, 0), (RAY_LCAP + 1, 3)):
        st = off_and_on(renderer, oracle, f"wide-{n}")[1][2]
        assert st["long_rays"] == 3 and st["scratch_rays"] == scratch
    st = off_and_on(renderer, oracle, "cloud-8193")[1][2]
    assert st["long_rays"] >= 5 and st["short_rays"] >= 5


# ---- 2. not both wrong ----
@pytest.mark.parametrize("name", ["g32-scattered"] + [f"stack-{k}" for k in (RAY_PL - 1, RAY_PL, RAY_PL + 1)]
                         + [f"wide-{n}" for n in (RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1)])
def test_indexed_bundle_against_the_oracle(renderer, oracle, name):
    g, o, d, eps = X.cases(oracle)[name]
    rad = off_and_on(renderer, oracle, name)[1][0]
    ref = S.oracle_radiance(oracle, o, d, g)
    lo, hi = S.kept_range(o, d, g, eps)
    err = np.abs(rad.astype(np.float64) - ref).max(1)
    print(name, "max err", err.max(), "peak", ref.max())
    assert ref.max() > 0.05
    assert (err <= S.tolerance(lo, hi, float(ref.max()))).all(), err.max()


# ---- 3. the index is used, and as modelled ----
@pytest.mark.parametrize("name", names())
def test_index_statistics_are_the_models(renderer, oracle, name):
    g, o, d, eps = X.cases(oracle)[name]
    st, ist = off_and_on(renderer, oracle, name)[1][2:]
    idx = X.Index(g, eps)
    tr = X.Traversal(idx, o, d)
    rays = len(d)
    print(name, ist, "model leaves", tr.leaves_kept(), "groups", tr.groups_kept(), "members <=", tr.members_tested_max())
    assert ist["indexed"] == 1 and ist["leaves"] == len(idx.leaves) and ist["groups"] == len(idx.groups)
    assert ist["groups_tested"] == rays * len(idx.groups)
    assert tr.groups_kept()[0] <= ist["groups_kept"] <= tr.groups_kept()[1]
    assert tr.leaves_kept()[0] <= ist["leaves_kept"] <= tr.leaves_kept()[1]
    assert ist["leaves_kept"] <= ist["leaves_tested"] <= rays * len(idx.leaves)
    assert ist["members_tested"] <= tr.members_tested_max()
    assert st["chunks_tested"] == 0 and st["members_tested"] == 0              # the chunk spheres were not consulted
    if name == "cloud-8193":
        assert (ist["leaves"], ist["groups"]) == (129, 3)
    if name == "g64-coherent":
        assert ist["leaves_kept"] / rays <= 4.0


# ---- 4. a ray's bits depend on the ray alone ----
def test_permuted_bundle_gives_the_permuted_result(renderer, oracle):
    g, o, d, eps = X.cases(oracle)["g32-scattered"]
    want = off_and_on(renderer, oracle, "g32-scattered")[1][0]
    renderer.set_gaussians(g)
    renderer.set_options(1, 1, eps)
    perm = np.random.default_rng(1).permutation(len(d))
    renderer.set_ray_index(1)
    try:
        got = renderer.radiance_rays(o[perm], d[perm])
    finally:
        renderer.set_ray_index(0)
    np.testing.assert_array_equal(got, want[perm])


# ---- 5. state ----
def test_scene_change_rebuilds_the_index(renderer, oracle, pkg):
    g1, o1, d1, _ = X.cases(oracle)["g16-coherent"]
    g2, o2, d2, _ = X.cases(oracle)["cloud-4097"]
    fresh = pkg.Renderer(0)
    try:
        fresh.set_gaussians(g2)
        want = fresh.radiance_rays(o2, d2, want_image=True)
    finally:
        fresh.close()
    renderer.set_gaussians(g1)
    renderer.set_options(1, 1, 1e-9)
    gen = pkg.lib().vrt_hip_state_generation(renderer._h)
    renderer.set_ray_index(1)
    assert pkg.lib().vrt_hip_state_generation(renderer._h) > gen      # a state change: holders of mirrors see it
    renderer.enable_stats(True)
    try:
        renderer.radiance_rays(o1, d1)
        assert renderer.ray_index_stats()["leaves"] == 4
        renderer.set_gaussians(g2)
        got = renderer.radiance_rays(o2, d2, want_image=True)
        assert renderer.ray_index_stats()["indexed"] == 1 and renderer.ray_index_stats()["leaves"] == 65
    finally:
        renderer.set_ray_index(0)
        renderer.enable_stats(False)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_mirror_shades_with_the_same_index(oracle, pkg):
    g, o, d, _ = X.cases(oracle)["g32-scattered"]
    src, dst = pkg.Renderer(0), pkg.Renderer(0)
    try:
        src.set_gaussians(g)
        want = src.radiance_rays(o, d, want_image=True)                # index off
        src.set_ray_index(1)
        assert pkg.lib().vrt_hip_copy_state(dst._h, src._h) == 0
        dst.enable_stats(True)
        got = dst.radiance_rays(o, d, want_image=True)
        ist = dst.ray_index_stats()
        src.enable_stats(True)
        src.radiance_rays(o, d)
        assert ist["indexed"] == 1 and ist == src.ray_index_stats()    # the same index: the same counts
    finally:
        src.close()
        dst.close()
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_scene_change_right_behind_an_indexed_bundle_in_flight(renderer, oracle):
    import torch
    g1, o, d, _ = X.cases(oracle)["g32-scattered"]
    g2, o2, d2, _ = X.cases(oracle)[f"stack-{RAY_PL + 1}"]
    o2 = np.tile(o2, (len(d2), 1))
    want1 = off_and_on(renderer, oracle, "g32-scattered")[0][0]
    want2 = off_and_on(renderer, oracle, f"stack-{RAY_PL + 1}")[0][0]
    renderer.set_gaussians(g1)
    renderer.set_options(1, 1, 1e-9)
    renderer.set_ray_index(1)
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o, d, o2, d2)]
            out1 = torch.zeros((len(d), 4), dtype=torch.float32, device="cuda")
            out2 = torch.zeros((len(d2), 4), dtype=torch.float32, device="cuda")
            st.synchronize()
            renderer.radiance_rays_device(len(d), t[0].data_ptr(), 1, t[1].data_ptr(), out1.data_ptr(), stream=st.cuda_stream)
            renderer.set_gaussians(g2)                                   # no synchronisation by the caller
            renderer.radiance_rays_device(len(d2), t[2].data_ptr(), 1, t[3].data_ptr(), out2.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
    finally:
        renderer.set_ray_index(0)
    assert want1.max() > 0.05 and want2.max() > 0.05
    np.testing.assert_array_equal(out1.cpu().numpy(), want1)
    np.testing.assert_array_equal(out2.cpu().numpy(), want2)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import oracle
import ray_index_scenes as X
from conftest import load_pkg
g, o, d, _ = X.cases(oracle)["g16-coherent"]
r = load_pkg().Renderer(0)
r.set_gaussians(g)
r.enable_stats(True)
rad = r.radiance_rays(o, d)
print("indexed", r.ray_index_stats()["indexed"], rad.tobytes().hex())
r.close()
"""


def test_environment_turns_the_index_on_at_creation(renderer, oracle):
    want = off_and_on(renderer, oracle, "g16-coherent")[0][0]
    env = dict(os.environ, VRT_HIP_RAY_INDEX="1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    word, flag, bits = p.stdout.strip().splitlines()[-1].split()
    assert (word, flag) == ("indexed", "1")
    assert bytes.fromhex(bits) == want.tobytes()


# ---- 6. the C++ example ----
def test_cpp_example_shades_twice_and_compares(tmp_path):
    """host/ray_bundle_example.cpp shades its stereo pair a second time after vrt::set_ray_index(true) and compares with memcmp."""
    p = subprocess.run([os.path.join(BIN, "ray_bundle_example")], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "ray index: identical" in p.stderr.splitlines()
    assert len(p.stdout.strip().splitlines()) == 2
