"""A float64 model of the ray bundles' Morton index (vrt_hip_set_ray_index, build_ray_index in csrc/vrt_hip_rays.cpp and the INDEXED
kernels of csrc/vrt_ray_kernel.hip) and the scenes that tests/test_gpu_ray_index.py shades with the index on and off;
tests/test_ray_index_scenes.py checks on the CPU that the model covers the cull rule and that the scenes exercise what they claim.

The index: Gaussians ordered by the Morton key of their centres (10 bits per axis over the bounding box of the centres, x in the lowest
bit of each triple, an axis of zero extent -> 0, ties by scene index); leaf spheres over 64 consecutive positions of that order (centre =
mid-point of the box of the members' centres, radius = max(distance + cull reach) with build_chunks_kernel's margins); group spheres
over 64 consecutive leaves; every sphere tested against the ray's LINE (ray_chunk_keeps).
"""
import numpy as np

import ray_bundle_scenes as S
from ray_bundle_scenes import RAY_PL, RAY_LCAP, CULL_EPS, EXP_FLOOR, Scene  # noqa: F401

LEAF = 64      # Morton positions per leaf sphere
GROUP = 64     # leaves per group sphere
CLOUD_SIZES = (1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 8193)   # bitmap word, leaf and group edges, ragged last leaf and group, three groups


# ---- the index ----
def _spread3(v):
    v = v.astype(np.uint32) & 0x3FF
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def morton_keys(g):
    mu = g["mu"][:, :3].astype(np.float64)
    finite = np.isfinite(mu).all(1)
    key = np.zeros(len(g), np.uint32)
    if finite.any():
        lo, hi = mu[finite].min(0), mu[finite].max(0)
        for a in range(3):
            ext = hi[a] - lo[a]
            if ext > 0:
                q = np.minimum(1023.0, np.floor((np.where(finite, mu[:, a], lo[a]) - lo[a]) / ext * 1024.0))
                key |= _spread3(q.astype(np.uint32)) << np.uint32(a)
    key[~finite] = 0
    return key


def morton_order(g):
    """perm[Morton position] = scene index: by key, ties by scene index."""
    return np.argsort(morton_keys(g), kind="stable").astype(np.uint32)


def cull_reach(g, cull_eps=CULL_EPS, exp_kind=1):
    """Distance from a ray's line beyond which the leaf spheres count a Gaussian as dropped: x = d^2 / (2 sigma^2) with
    0.999 x - 1e-3 > cull_x (build_chunks_kernel)."""
    sigma = g["sigma"].astype(np.float64)
    q = np.abs(sigma * g["magnitude"].astype(np.float64))
    cull_x = np.full(len(g), EXP_FLOOR[exp_kind])
    if cull_eps > 0:
        with np.errstate(divide="ignore"):
            cull_x = np.minimum(cull_x, np.log(q / (cull_eps * min(1.0, 4096.0 / max(len(g), 1)))))
    cull_x[q == 0] = -np.inf
    xr = cull_x + 1e-3
    return np.where(xr > 0, np.sqrt(np.maximum(xr, 0) * 2.0 * sigma * sigma / 0.999), 0.0)


def _bound(centres, radii, size):
    """Spheres (x, y, z, rho) over runs of `size` rows: box mid-point, the farthest row plus its radius, the kernels' margins."""
    out = np.zeros(((len(centres) + size - 1) // size, 4))
    for k in range(len(out)):
        c, r = centres[k * size:(k + 1) * size], radii[k * size:(k + 1) * size]
        mid = 0.5 * (c.min(0) + c.max(0))
        rho = (np.linalg.norm(c - mid, axis=1) + r).max()
        out[k] = (*mid, rho * 1.0001 + 1e-6 * (1.0 + np.abs(mid).sum()))
    return out


class Index:
    def __init__(self, g, cull_eps=CULL_EPS, exp_kind=1):
        self.n = len(g)
        self.perm = morton_order(g)
        mu = g["mu"][:, :3].astype(np.float64)[self.perm]
        self.leaves = _bound(mu, cull_reach(g, cull_eps, exp_kind)[self.perm], LEAF)
        self.groups = _bound(self.leaves[:, :3], self.leaves[:, 3], GROUP)
        self.leaf_of = np.empty(self.n, np.int64)                    # scene index -> its leaf
        self.leaf_of[self.perm] = np.arange(self.n) // LEAF
        self.leaf_size = np.bincount(np.arange(self.n) // LEAF, minlength=len(self.leaves))


def sphere_keeps(spheres, origins, dirs):
    """(lo, mid, hi), each [rays, spheres] bool: ray_chunk_keeps in float64, and between what the float32 evaluation can fall.  d^2 - t^2
    is a difference of numbers of size d^2 formed in float32 (8 * 2^-24 d^2, as kept_range) and the device's radius is the model's
    within a few float32 roundings (1e-5 relative is generous): a sphere within that of the line may go either way."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    a = spheres[None, :, :3] - o[:, None, :]
    d2 = (a * a).sum(2)
    t = (a * d[:, None, :]).sum(2)
    core = d2 - t * t - 8e-6 * d2
    band = 8.0 * 2.0 ** -24 * d2
    rho = spheres[None, :, 3]

    def keeps(extra, scale):
        return ~(np.sqrt(np.maximum(0.0, core + extra)) * 0.9999 > rho * scale)
    return keeps(band, 1.0 - 1e-5), keeps(0.0, 1.0), keeps(-band, 1.0 + 1e-5)


class Traversal:
    """What the rays keep of an Index: per ray and leaf, with the ray's OWN group test applied, as (lo, mid, hi)."""
    def __init__(self, index, origins, dirs):
        self.index = index
        self.group = sphere_keeps(index.groups, origins, dirs)
        own = sphere_keeps(index.leaves, origins, dirs)
        of = np.arange(len(index.leaves)) // GROUP
        self.leaf = tuple(l & g[:, of] for l, g in zip(own, self.group))
        self.rays = len(self.leaf[0])

    def groups_kept(self):
        """(lo, hi) sums over the rays"""
        return int(self.group[0].sum()), int(self.group[2].sum())

    def leaves_kept(self):
        return int(self.leaf[0].sum()), int(self.leaf[2].sum())

    def members_tested_max(self):
        """Upper count of the short kernel's member tests: every ray of a wave of 64 consecutive rays counts the members of every
        leaf that SOME ray of the wave may keep."""
        total = 0
        for r0 in range(0, self.rays, 64):
            wave = self.leaf[2][r0:r0 + 64]
            total += len(wave) * int(self.index.leaf_size[wave.any(0)].sum())
        return total

    def covers(self, keep):
        """keep [rays, N] bool (ray_bundle_scenes.kept): every kept Gaussian lies in a leaf -- hence a group -- that the ray keeps
        for certain."""
        return bool(self.leaf[0][:, self.index.leaf_of][keep].all())


# ---- scenes ----
def shuffled(g, seed, fixed=()):
    """g in a seeded random scene order; the Gaussians at the indices `fixed` stay where they are."""
    rng = np.random.default_rng(seed)
    free = np.setdiff1d(np.arange(len(g)), np.asarray(fixed, np.int64))
    order = np.arange(len(g))
    order[free] = rng.permutation(free)
    return g[order]


def shuffled_stack_with_side(oracle, k):
    """S.stack_with_side in a random scene order.  The stack lies on the z axis, where Morton order = scene order: only the shuffle makes
    the indexed kernels put a list back into scene order."""
    return shuffled(S.stack_with_side(oracle, k), 7700 + k)


def shuffled_wide_stack(oracle, cap, n):
    """S.wide_stack with everything but its markers in a random scene order: the markers stay at the list positions 0, cap - 1, cap, n - 1
    where an off-by-one of the bitmap read-off at the capacity bites."""
    sc = S.wide_stack(oracle, cap, n)
    return Scene(g=shuffled(sc.g, 8800 + n, sc.markers), n=n, cap=cap, markers=sc.markers)


def cloud(oracle, n, seed=None):
    """n small Gaussians at random in a box in front of the rays' origin; sigma shrinks with n so that a ray aimed at one of them keeps
    a handful to a few dozen -- both kernels at the larger sizes."""
    rng = np.random.default_rng(4100 + n if seed is None else seed)
    mu = rng.uniform([-1.0, -1.0, 0.0], [1.0, 1.0, 2.0], size=(n, 3))
    sigma = rng.uniform(0.8, 1.2, n) * np.clip(1.0 / np.sqrt(n), 0.011, 0.1)
    mag = rng.uniform(0.3, 0.9, n) / (S.SQRT_2PI * sigma)
    return oracle.gaussians(rng.uniform(0.1, 1.0, size=(n, 4)), mu, sigma, mag)


def cloud_rays(g):
    return S.coherent_rays(g, count=70, seed=len(g))              # two waves, the second ragged


def cases(oracle):
    """Every (name, scene, origins, dirs, cull_eps) the GPU tests shade with the index on and off.  Built once."""
    if not _cases:
        g16, g32, g64 = (oracle.grid_scene(d) for d in (16, 32, 64))
        add = lambda name, g, od, eps=CULL_EPS: _cases.__setitem__(name, (g, od[0], od[1], eps))  # noqa: E731
        add("g16-coherent", g16, S.coherent_rays(g16))
        add("g16-coherent-nocull", g16, S.coherent_rays(g16), 0.0)
        add("g32-scattered", g32, S.scattered_rays(g32))
        add("g64-centre", g64, S.centre_rays(g64))
        add("g64-coherent", g64, S.coherent_rays(g64, 130, seed=11))
        for k in (RAY_PL - 1, RAY_PL, RAY_PL + 1):
            add(f"stack-{k}", shuffled_stack_with_side(oracle, k), S.stack_rays())
        for n in (RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1):
            add(f"wide-{n}", shuffled_wide_stack(oracle, RAY_LCAP, n).g, S.wide_rays())
        for n in CLOUD_SIZES:
            c = cloud(oracle, n)
            add(f"cloud-{n}", c, cloud_rays(c))
    return _cases


_cases = {}
