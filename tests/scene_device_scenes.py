"""Scenes and helpers of tests/test_gpu_scene_device.py: the scene set from device memory (vrt_hip_set_gaussians_device,
csrc/vrt_scene_kernel.hip) against the same scene set through the host.  tests/test_scene_device_scenes.py checks on the CPU that the
crafted scenes do what they claim, so that the GPU tests do not pass on vacuous inputs.

The device path has three things to get exactly right: the nine columns (any scene shows a slip), albedo_scale (the largest finite
|albedo|, at least 1: block_scenes' factor scenes move the block kernel's statistics with it), and the Morton index built by kernels --
the same double-precision keys, the same order among EQUAL keys (a stable sort), an axis without extent, centres that are not finite.
"""
import numpy as np

import block_scenes as B
import ray_bundle_scenes as S
import ray_index_scenes as X
from ray_index_scenes import LEAF, GROUP, morton_keys, morton_order  # noqa: F401

SIZES = (0, 1, 63, 64, 65, 130, 1000)        # nothing, one, a leaf's edge from both sides, three leaves, several blocks of the ingest kernel
ORIGIN = np.array([0.0, 0.0, -4.0], np.float32)
SAMPLES = np.linspace(0.5, 7.0, 7).astype(np.float32)
LEVELS = np.array([0.9, 0.5, 0.1], np.float32)


def packed(g):
    """The four arrays the device setter takes: mu [n, 3], albedo [n, 4] (column 3 = alpha), sigma [n], magnitude [n], float32."""
    return (np.ascontiguousarray(g["mu"][:, :3], np.float32), np.ascontiguousarray(g["albedo"], np.float32),
            np.ascontiguousarray(g["sigma"], np.float32), np.ascontiguousarray(g["magnitude"], np.float32))


def cloud(oracle, n):
    """ray_index_scenes' seeded cloud in the box [-1, 1]^2 x [0, 2]; n = 0: the empty scene."""
    return X.cloud(oracle, n, seed=6100 + n) if n else oracle.gaussians(np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(0), np.zeros(0))


def rays(count=130, seed=17):
    """count rays from ORIGIN through seeded points of the clouds' box: they do not depend on the scene, so every scene -- the empty
    one too -- is shaded by the same bundle.  Three waves, the last one ragged."""
    rng = np.random.default_rng(seed)
    target = rng.uniform([-1.0, -1.0, 0.0], [1.0, 1.0, 2.0], size=(count, 3))
    return ORIGIN, S.normalise(target - ORIGIN.astype(np.float64)).astype(np.float32)


def seeded_grad(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


# ---- the crafted scenes of the index ----
def tie_scene(oracle, n=130, first=58, last=70):
    """A cloud in which the Gaussians at the Morton positions first .. last - 1 share one centre, hence one key: a run of equal keys
    across position 64, the border of the first two leaves.  Their scene indices are scattered, so only a STABLE sort puts them where
    morton_order does."""
    g = X.cloud(oracle, n, seed=6200).copy()
    run = morton_order(g)[first:last]
    g["mu"][run] = g["mu"][run[0]]
    return g


def flat_scene(oracle, n=100):
    """A cloud in the plane y = 0.25: an axis of zero extent, whose 10 bits are 0."""
    g = X.cloud(oracle, n, seed=6300).copy()
    g["mu"][:, 1] = 0.25
    return g


NONFINITE = 70      # more than a leaf: the key of a centre that is not finite is 0, so they fill leaf 0 and reach into leaf 1


def nonfinite_scene(oracle, n=300):
    """A cloud of five leaves, NONFINITE of whose centres are not finite -- NaN, +inf and -inf, in every coordinate."""
    g = X.cloud(oracle, n, seed=6400).copy()
    bad = np.random.default_rng(6401).choice(n, NONFINITE, replace=False)
    for k, i in enumerate(bad):
        g["mu"][i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    return g


def open_leaves(g):
    """The leaves build_ray_index opens (a NaN radius): those with a member whose centre is not finite or whose sigma is NaN."""
    bad = ~np.isfinite(g["mu"][:, :3]).all(1) | np.isnan(g["sigma"])
    return np.unique(np.flatnonzero(bad[morton_order(g)]) // LEAF)


def index_scenes(oracle):
    """name -> scene, built once: the crafted ones, the sizes around a leaf, and 4097 Gaussians (65 leaves: two groups)."""
    if not _index_scenes:
        _index_scenes.update({"ties": tie_scene(oracle), "flat": flat_scene(oracle), "nonfinite": nonfinite_scene(oracle),
                              "cloud-4097": X.cloud(oracle, 4097)})
        _index_scenes.update({f"cloud-{n}": cloud(oracle, n) for n in (0, 1, 64, 65)})
    return _index_scenes


_index_scenes = {}
INDEX_NAMES = ("ties", "flat", "nonfinite", "cloud-4097", "cloud-0", "cloud-1", "cloud-64", "cloud-65")


# ---- albedo_scale ----
def albedo_scale_bits(albedo):
    """The ingest kernel's rule: the maximum over the BIT PATTERNS of |albedo| that are finite (non-negative floats order as unsigned
    integers), then max(1, that float)."""
    b = np.ascontiguousarray(albedo, np.float32).view(np.uint32).ravel() & np.uint32(0x7FFFFFFF)
    b = b[b < 0x7F800000]
    m = np.array([b.max() if b.size else 0], np.uint32).view(np.float32)[0]
    return float(max(np.float32(1.0), m))


def all_nan_albedo(oracle):
    """block_scenes' plain factor scene with every albedo NaN: nothing finite, the scale stays 1."""
    sc = B.Scene(B.scene(oracle, ("factors", "plain")))
    g = sc.g.copy()
    g["albedo"][:] = np.nan
    sc.update(g=g, kind="albedo-nan")
    return sc


def nan_is_the_only_large_albedo(oracle):
    g = cloud(oracle, 65).copy()
    g["albedo"][7, 2] = np.nan
    return g


def dimmed(sc):
    """The factor scene with every albedo back in [0, 1]: the scale returns to 1."""
    out = B.Scene(sc)
    g = sc.g.copy()
    a = g["albedo"]
    a[~np.isfinite(a) | (np.abs(a) > 1.0)] = 0.5
    out.update(g=g, kind=str(sc.get("kind")) + "-dimmed")
    return out
