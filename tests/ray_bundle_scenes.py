"""Scenes and rays for the ray-bundle path (vrt_hip_radiance_rays*, csrc/vrt_ray_kernel.hip): tests/test_gpu_ray_bundles.py shades
them on the GPU, tests/test_ray_bundle_scenes.py checks with the oracle alone that they test what they claim.

The path has two kernels and two capacities (csrc/vrt_kernels.h):
  RAY_PL   32    per-ray list of the lane = ray kernel; a ray that keeps more goes to the one-wave-per-ray kernel
  RAY_LCAP 1024  survivors the one-wave-per-ray kernel holds in LDS; beyond that its list continues in device memory
A ray keeps Gaussian j unless x > cull_x_j: x = (|oc|^2 - mubar^2) / (2 sigma_j^2), cull_x_j = ln(sigma_j mag_j / eps_eff),
eps_eff = cull_eps min(1, 4096 / N), at most the point where Exp gives exactly 0 (87.3 for vcl_exp).  `kept` restates that in float64.
By DESIGN.md section 4 a ray then loses less than 3 cull_eps min(N, 4096) = 1.23e-5 at the default cull_eps.
"""
import numpy as np

from boundary_scenes import SQRT_2PI, TOL, TOL_NOCULL, MARKER_FACTOR, Scene, marker_indices  # noqa: F401

RAY_PL, RAY_LCAP = 32, 1024
CULL_EPS = 1e-9
CULL_BOUND = 3 * CULL_EPS * 4096     # 1.23e-5: what a ray can lose to the cull at the default cull_eps, for any N
EXP_FLOOR = {0: 104.0, 1: 87.3}      # oracle.EXP_LIBM, EXP_VCL: Exp(-x) is exactly 0 beyond


def kept(origins, dirs, g, cull_eps=CULL_EPS, exp_kind=1):
    """[rays, N] bool: the cull rule in float64.  origins: [3] or [rays, 3]."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    oc = g["mu"][:, :3].astype(np.float64)[None, :, :] - o[:, None, :]
    t = (oc * d[:, None, :]).sum(2)
    sigma = g["sigma"].astype(np.float64)
    x = ((oc * oc).sum(2) - t * t) / (2.0 * sigma * sigma)[None, :]
    q = np.abs(sigma * g["magnitude"].astype(np.float64))
    cull_x = np.full(len(g), EXP_FLOOR[exp_kind])
    if cull_eps > 0:
        eps_eff = cull_eps * min(1.0, 4096.0 / max(len(g), 1))
        with np.errstate(divide="ignore"):
            cull_x = np.minimum(cull_x, np.log(q / eps_eff))
    cull_x[q == 0] = -np.inf
    return ~(x > cull_x[None, :])


def kept_range(origins, dirs, g, cull_eps=CULL_EPS, exp_kind=1):
    """(lo, hi) per ray: the list lengths between which the float32 evaluation of the rule can fall.  x is a difference of two
    numbers of size |oc|^2 formed in float32 (a few ulp each: 8 * 2^-24 |oc|^2 / (2 sigma^2) of x is generous), so a Gaussian
    within that of its threshold may go either way; everything else is decided."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    oc = g["mu"][:, :3].astype(np.float64)[None, :, :] - o[:, None, :]
    t = (oc * d[:, None, :]).sum(2)
    sigma = g["sigma"].astype(np.float64)
    scale = 1.0 / (2.0 * sigma * sigma)[None, :]
    x = ((oc * oc).sum(2) - t * t) * scale
    band = 8.0 * 2.0 ** -24 * (oc * oc).sum(2) * scale + 1e-5 * np.abs(x)
    q = np.abs(sigma * g["magnitude"].astype(np.float64))
    cull_x = np.full(len(g), EXP_FLOOR[exp_kind])
    if cull_eps > 0:
        with np.errstate(divide="ignore"):
            cull_x = np.minimum(cull_x, np.log(q / (cull_eps * min(1.0, 4096.0 / max(len(g), 1)))))
    cull_x[q == 0] = -np.inf
    return (~(x + band > cull_x[None, :])).sum(1), (~(x - band > cull_x[None, :])).sum(1)


def tolerance(lo, hi, peak, nocull=False):
    """Per ray, from kept_range's (lo, hi): a ray that the lane = ray kernel shades for certain (hi <= RAY_PL) is summed like the
    reference (TOL, or TOL_NOCULL with the cull off); the one-wave-per-ray kernel sums in another order (TOL max(1, peak), as
    boundary_scenes.tolerance) -- also allowed to the rare ray whose float32 list length may fall on either side of RAY_PL."""
    return np.where(np.asarray(hi) <= RAY_PL, TOL_NOCULL if nocull else TOL, TOL * max(1.0, float(peak)))


def normalise(d):
    """float32 unit directions: what the GPU and the oracle both get."""
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


def coherent_rays(g, count=130, seed=11, origin=(0.0, 0.0, -4.0)):
    """One origin; ray k aims at the centre of a Gaussian (spread over the scene) with a jitter of about sigma.  (The CLI camera's
    pinhole rays mostly miss a grid scene: they pass between the Gaussians.)"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(g), size=count, replace=count > len(g))
    target = g["mu"][pick, :3].astype(np.float64) + rng.normal(size=(count, 3)) * g["sigma"][pick, None]
    o = np.asarray(origin, np.float32)
    return o, normalise(target - o.astype(np.float64))


def scattered_rays(g, count=32, seed=5, radius=4.0):
    """Every ray its own origin on a sphere around the scene's centre, aimed at a uniform point of the scene's bounding box: from
    head-on to grazing along the grid's plane, so the lists run from a handful to far beyond RAY_PL."""
    rng = np.random.default_rng(seed)
    mu = g["mu"][:, :3].astype(np.float64)
    lo, hi = mu.min(0), mu.max(0)
    v = rng.normal(size=(count, 3))
    o = ((lo + hi) / 2 + radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    target = rng.uniform(lo, hi, size=(count, 3))
    return o, normalise(target - o.astype(np.float64))


def centre_rays(g, count=64, seed=3, origin=(0.0, 0.0, -4.0)):
    """`count` rays from one origin through the centres of Gaussians near the middle of the scene (one coherent wave)."""
    mu = g["mu"][:, :3].astype(np.float64)
    near = np.argsort(np.linalg.norm(mu - mu.mean(0), axis=1), kind="stable")[:count]
    o = np.asarray(origin, np.float32)
    return o, normalise(mu[np.sort(near)] - o.astype(np.float64))


# ---- RAY_PL: K Gaussians in a row on the z axis; an axial ray keeps exactly K, one aimed 0.6 off none ----
STACK_ORIGIN = np.array([0.0, 0.0, -4.0], np.float32)


def stack(oracle, k, seed=None):
    rng = np.random.default_rng(3200 + k if seed is None else seed)
    mu = np.stack([np.zeros(k), np.zeros(k), np.linspace(0.2, 1.8, k)], 1)
    sigma = np.full(k, 0.05)
    mag = np.full(k, 2.0 / (k * SQRT_2PI * 0.05))
    alb = rng.uniform(0.1, 1.0, size=(k, 4))
    return oracle.gaussians(alb, mu, sigma, mag)


def stack_rays(nmiss=62):
    """[axial, aimed 0.02 off the axis at depth 1, nmiss rays aimed 0.6 off the axis all around it]."""
    ang = np.arange(nmiss) * (2 * np.pi / max(nmiss, 1))
    target = np.concatenate([[[0.0, 0.0, 1.0], [0.02, 0.0, 1.0]], np.stack([0.6 * np.cos(ang), 0.6 * np.sin(ang), np.ones(nmiss)], 1)])
    return STACK_ORIGIN, normalise(target - STACK_ORIGIN.astype(np.float64))


def stack_with_side(oracle, k):
    """The stack of k and, behind it in the list, a column of 5 Gaussians on the line (0.6, 0, z): of stack_rays() the two axial
    rays keep the k of the stack alone, the ray aimed at (0.6, 0, 1) and its neighbours keep some of the column alone -- wave-mates
    with radiance of their own.  stack_with_side(k + 1)[:k] + its column is stack_with_side(k) but for one Gaussian the
    wave-mates do not see: the magnitudes are those of k + 1 in both (see one_over_pair)."""
    g = stack(oracle, k)
    side = oracle.gaussians(np.linspace(0.2, 1.0, 20).reshape(5, 4), np.stack([np.full(5, 0.6), np.zeros(5), np.linspace(0.6, 1.4, 5)], 1),
                            np.full(5, 0.05), np.full(5, 1.5))
    return np.concatenate([g, side])


def one_over_pair(oracle):
    """(scene whose axial rays keep RAY_PL, the same scene with one more Gaussian at the end of the stack): RAY_PL + 1 on the axis."""
    over = stack_with_side(oracle, RAY_PL + 1)
    return np.delete(over, RAY_PL), over


# ---- RAY_LCAP: n wide, faint Gaussians around the z axis that every near-axial ray keeps, with markers ----
def wide_stack(oracle, cap, n):
    """boundary_scenes.cloud's Gaussians (sigma ~ 1, optical depth of the whole cloud ~ 1) with strong markers on the axis at the
    indices where an off-by-one at `cap` bites: 0, cap - 1, cap, n - 1."""
    rng = np.random.default_rng(1000 * cap + n)
    mu = rng.normal(size=(n, 3)) * 0.15 + np.array([0, 0, 1.0])
    sigma = rng.uniform(0.9, 1.3, n)
    mag = rng.uniform(0.4, 1.6, n) / (n * SQRT_2PI * sigma)
    alb = rng.uniform(0.1, 1.0, size=(n, 4))
    markers = marker_indices(cap, n)
    for j, k in enumerate(markers):
        mu[k] = (0.0, 0.0, 0.55 + 0.9 * (j + 0.5) / len(markers))
        sigma[k] = 0.5
        mag[k] = 0.25 / (SQRT_2PI * 0.5)
        alb[k] = [(1.0, 0.3, 0.2, 1.0), (0.2, 1.0, 0.3, 1.0), (0.3, 0.2, 1.0, 1.0), (1.0, 1.0, 0.2, 1.0)][j % 4]
    return Scene(g=oracle.gaussians(alb, mu, sigma, mag), n=n, cap=cap, markers=markers)


def wide_rays():
    """The axial ray and two slightly off it (every one keeps the whole wide stack)."""
    target = np.array([[0.0, 0.0, 1.0], [0.05, 0.02, 1.0], [-0.03, 0.06, 1.0]])
    return STACK_ORIGIN, normalise(target - STACK_ORIGIN.astype(np.float64))


def oracle_radiance(oracle, origins, dirs, g, exp_kind=1, erf_kind=1, rays=None):
    """oracle.radiance per ray over the WHOLE scene, with the float32 origins and directions the GPU gets.  [rays, 4]."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    rays = range(len(d)) if rays is None else rays
    return np.stack([oracle.radiance(o[r if len(o) > 1 else 0], d[r], g, exp_kind, erf_kind) for r in rays])
