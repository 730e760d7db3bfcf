"""A float64 model of the sorted ray bundles (vrt_hip_set_ray_sort, csrc/vrt_ray_sort_kernel.hip, ray_short_slot in
csrc/vrt_ray_cull.hpp) and the bundles that tests/test_gpu_ray_sort.py shades with the sort on and off; tests/test_ray_sort_scenes.py
checks on the CPU that the model says what the sort is for and that the cases can see the ways it can go wrong.

The sort: every ray gets the key (min(first, 0xFFFF) << 16) | min(last, 0xFFFF), first / last = the lowest / highest bounding sphere
its OWN tests keep -- leaf spheres in Morton position behind the ray's own group test with the index on (ray_index_scenes.Traversal),
the chunk spheres over 64 consecutive scene indices with it off (chunk_spheres below: build_chunks_kernel's arithmetic, which the
index's leaves share, over the rows in scene order) -- and 0xFFFFFFFF when it keeps none; the rays are sorted by key, ties in ray
order, and lane l of wave w of a lane = ray kernel takes ray order[64 w + l].  A wave tests the members of every sphere that SOME
lane of it keeps; results are written at the ray id.
"""
import numpy as np

import ray_bundle_scenes as S
import ray_index_scenes as X
from ray_index_scenes import Index, Traversal, cloud, cloud_rays, shuffled_wide_stack, sphere_keeps  # noqa: F401
from ray_bundle_scenes import RAY_PL, RAY_LCAP, CULL_EPS  # noqa: F401

NONE = 0xFFFFFFFF
SIZES = (0, 1, 64, 65, 130, 1024)     # nothing, one lane, one full wave (not sorted), two waves, three with a last wave of two lanes, sixteen
# The main case: cloud(4097) (65 leaves in 2 groups) and rays aimed at random Gaussians of it.  A leaf of that cloud is a cube of edge
# 0.5 whose sphere reaches well into its neighbours: a ray keeps 20 of the 65 leaves, and a sorted wave of 1024 such rays (54 distinct
# keys, 16 waves) still keeps 0.57 of what a shuffled wave keeps, of 2048 rays 0.51.  4096 is the smallest power of two at which the
# sorted order's UPPER member count is at most half of the shuffled order's LOWER one (0.49): tests/test_ray_sort_scenes.py asserts it.
MAIN_N, MAIN_RAYS, MAIN_SEED, SHUFFLE_SEED = 4097, 4096, 29, 61


def chunk_spheres(g, cull_eps=CULL_EPS, exp_kind=1):
    """The chunk spheres of a scene: the index's leaf arithmetic over runs of 64 rows in SCENE order."""
    return X._bound(g["mu"][:, :3].astype(np.float64), X.cull_reach(g, cull_eps, exp_kind), 64)


class Spheres:
    """What the rays' own tests keep of the spheres the bundle's cull will use, as (lo, mid, hi) [rays, spheres] bool, and the
    members of every sphere."""
    def __init__(self, g, origins, dirs, indexed, cull_eps=CULL_EPS, group_test=True, leaf_test=True):
        n = len(g)
        self.size = np.bincount(np.arange(n) // 64, minlength=(n + 63) // 64)
        if indexed:
            idx = Index(g, cull_eps)
            tr = Traversal(idx, origins, dirs)
            of = np.arange(len(idx.leaves)) // X.GROUP
            own = sphere_keeps(idx.leaves, origins, dirs)
            if group_test and leaf_test: self.keep = tr.leaf
            elif leaf_test: self.keep = own                                     # WRONG: the ray's own group test is left out
            else: self.keep = tuple(gk[:, of] for gk in tr.group)               # WRONG: every leaf of a kept group
        else:
            self.keep = sphere_keeps(chunk_spheres(g, cull_eps), origins, dirs)
        self.rays = len(self.keep[0])

    def keys(self, which=1):
        """u32 [rays]: the key by the lo (0), mid (1) or hi (2) set."""
        return keys_of(self.keep[which])

    def bracket_ok(self, keys):
        """[rays] bool: the key is one the float32 tests can give -- the kept set K lies between lo and hi, first = min K, last = max K."""
        lo, hi = self.keep[0], self.keep[2]
        ns = lo.shape[1]
        keys = np.asarray(keys, np.int64)
        col = np.arange(ns)
        big = ns + 1
        first_min = np.where(hi.any(1), np.where(hi, col, big).min(1), big)     # the lowest sphere K can hold
        first_max = np.where(lo.any(1), np.where(lo, col, big).min(1), ns - 1)  # ... and the highest its minimum can be
        last_min = np.where(lo.any(1), np.where(lo, col, -1).max(1), 0)
        last_max = np.where(hi.any(1), np.where(hi, col, -1).max(1), -1)
        none = keys == NONE
        first, last = keys >> 16, keys & 0xFFFF
        clamp = lambda v: np.minimum(v, 0xFFFF)  # noqa: E731
        some = (clamp(first_min) <= first) & (first <= clamp(first_max)) & (clamp(last_min) <= last) & (last <= clamp(last_max)) & hi.any(1)
        return np.where(none, ~lo.any(1), some)

    def members_tested(self, order, which, last_wave=True):
        """The short kernel's member tests under `order` (slot -> ray id) by the lo (0) or hi (2) set: every ray of a wave of 64
        consecutive slots counts the members of every sphere that SOME ray of the wave keeps."""
        order = np.asarray(order, np.int64)
        total = 0
        stop = len(order) if last_wave else len(order) // 64 * 64                # WRONG without: the ragged last wave is dropped
        for s0 in range(0, stop, 64):
            wave = self.keep[which][order[s0:s0 + 64]]
            total += len(wave) * int(self.size[wave.any(0)].sum())
        return total


def keys_of(keep):
    ns = keep.shape[1]
    col = np.arange(ns)
    first = np.where(keep, col, ns).min(1) if ns else np.zeros(len(keep), np.int64)
    last = np.where(keep, col, -1).max(1) if ns else np.zeros(len(keep), np.int64)
    key = (np.minimum(first, 0xFFFF).astype(np.int64) << 16) | np.minimum(np.maximum(last, 0), 0xFFFF)
    return np.where(keep.any(1), key, NONE).astype(np.uint32)


def sort_order(keys, stable=True):
    """order[slot] = ray id: by key, ties in ray order.  stable=False (WRONG): ties in descending ray order."""
    keys = np.asarray(keys, np.int64)
    if stable:
        return np.argsort(keys, kind="stable").astype(np.uint32)
    n = len(keys)
    return (n - 1 - np.argsort(keys[::-1], kind="stable")).astype(np.uint32)


def order_faults(order, keys):
    """What is wrong with `order` as the sorted order of `keys` (by ray id): a list of words, empty when it is the stable sort."""
    order = np.asarray(order, np.int64)
    keys = np.asarray(keys, np.int64)
    faults = []
    if len(order) != len(keys) or not np.array_equal(np.sort(order), np.arange(len(keys))):
        return ["not a permutation"]
    k = keys[order]
    if (np.diff(k) < 0).any(): faults.append("keys descend")
    if ((np.diff(k) == 0) & (np.diff(order) < 0)).any(): faults.append("ties out of ray order")
    none = k == NONE
    if none.any() and not none[np.argmax(none):].all(): faults.append("a ray without a sphere is not last")
    return faults


def shade(values, order, at_ray=True, last_wave=True):
    """The bundle's output under `order`: slot s works on ray order[s] and writes values[order[s]] at out[order[s]] -- the identity,
    whatever the order.  at_ray=False (WRONG): written at out[s]; last_wave=False (WRONG): the ragged last wave never runs.  Unwritten
    words are -1."""
    order = np.asarray(order, np.int64)
    values = np.asarray(values)
    out = np.full(len(values), -1, values.dtype)
    stop = len(order) if last_wave else len(order) // 64 * 64
    slots = np.arange(stop)
    out[order[:stop] if at_ray else slots] = values[order[:stop]]
    return out


# ---- bundles ----
def aimed_rays(g, count, seed, per_ray_origin=False):
    """`count` rays aimed at random Gaussians of g (with a jitter of about sigma): from one origin, or every ray from an origin of its
    own on a sphere around the scene.  Neighbours in the bundle share nothing."""
    if not per_ray_origin:
        return S.coherent_rays(g, count=count, seed=seed)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(g), size=count, replace=count > len(g))
    target = g["mu"][pick, :3].astype(np.float64) + rng.normal(size=(count, 3)) * g["sigma"][pick, None]
    v = rng.normal(size=(count, 3))
    o = (np.array([0.0, 0.0, 1.0]) + 4.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return o, S.normalise(target - o.astype(np.float64))


def shuffled_rays(o, d, seed=SHUFFLE_SEED):
    """(origins, dirs, perm): the bundle under a seeded permutation; ray k of the result is ray perm[k] of the argument."""
    perm = np.random.default_rng(seed).permutation(len(d))
    return (o if np.ndim(o) == 1 else o[perm]), d[perm], perm


def main_case(oracle, count=MAIN_RAYS):
    """(g, origins, dirs): cloud(4097) and `count` rays aimed at random Gaussians of it from one origin."""
    g = cloud(oracle, MAIN_N)
    o, d = aimed_rays(g, count, MAIN_SEED)
    return g, o, d


def wide_rays(count, seed):
    """`count` rays from the stack's origin: every other one close to the axis (keeps the whole wide stack), the rest spread far from
    it (keep less, down to nothing) -- long and short rays interleaved, so that a sorted short kernel queues ray ids out of slot order."""
    rng = np.random.default_rng(seed)
    spread = np.where(np.arange(count) % 2 == 0, 0.04, 6.0)[:, None]
    target = np.concatenate([rng.normal(size=(count, 2)) * spread, np.ones((count, 1))], 1)
    return S.STACK_ORIGIN, S.normalise(target - S.STACK_ORIGIN.astype(np.float64))


WIDE = tuple((cap, n) for cap in (RAY_PL, RAY_LCAP) for n in (cap - 1, cap + 1))


def wide_case(oracle, cap, n, count=130):
    g = shuffled_wide_stack(oracle, cap, n).g
    o, d = wide_rays(count, 100 * cap + n)
    return g, o, d
