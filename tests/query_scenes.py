"""Scenes, float64 models and derived bounds for the point queries (csrc/vrt_query_kernel.hip behind csrc/vrt_hip_query.cpp:
transmittance, transmittance_rays, transmittance_step, density, radiance).  tests/test_gpu_queries.py runs them on the GPU,
tests/test_query_scenes.py checks with the oracle and the models alone that they test what they claim.  No GPU here.

Scenes (`scene(n)`): seeded, sigma in [0.1, 0.6], centres in the box |x|, |y| <= 1, -1 <= z <= 2, rays from near (0, 0, -3) towards +z:
|mu - o| <= 6 for every ray and Gaussian (asserted).  Every scene of n >= 5 starts with five Gaussians placed against ray 0
(`MARKERS`): [0] magnitude 0, [1] negative magnitude, [2] behind the origin, [3] its centre within sigma / 10 of the ray, [4] the origin
inside it.  A marker moves a checked value by at least ten tolerances when it is left out -- for [0], whose term is exactly 0, when it is
given the magnitude 1 instead (tests/test_query_scenes.py::test_markers).

Models, in float64 from the float32 inputs the GPU gets, with math.erf (depth_bundle_scenes.erf) or the Abramowitz-Stegun form the AS
pairs integrate with (erf_as).  Each returns (value, bound); the bound is what float32 evaluation in ANY order of the reference's
formula may differ from the float64 value, u = 2^-24 being the relative error of one float32 operation:

  geometry of (ray, Gaussian j):  c = mu_j - o, mubar = c.d, d2 = |c|^2 - mubar^2, x = d2 / (2 sigma^2), m = mubar r, r = 1 / (sqrt2 sigma)
    d(mubar) <= 4 u |c| |d|        (c rounded, three products, two sums)
    d(d2)    <= 16 u |c|^2          (|c|^2: 5 u |c|^2; mubar^2: 2 |mubar| d(mubar) + u mubar^2 <= 9 u |c|^2; the difference itself: the
                                     cancellation the comment above dot3_ref describes -- d2 ~ sigma^2 from two numbers ~ |c|^2)
    d(x)     <= d(d2) / (2 sigma^2) + 4 u x
  weight w = sigma mag K exp(-x), K = 1 / 0.79788456:  relative error  expm1(d(x)) + EXP_REL + 6 u
  erf arguments a1 = -m, a2 = s r - m:   d(a1) = d(mubar) r + 3 u |m|,   d(a2) = d(a1) + d(s) r + 3 u |s r| + u |a2|
  Erf: |Erf32(a + e) - Erf64(a)| <= ERF_ABS + the change of the model's own Erf over [a - e, a + e] (evaluated for erf_as, which is
    monotone; 2 / sqrt(pi) exp(-max(0, |a| - e)^2) e for erf)
  exponent E = sum_j w_j (Erf(a1_j) - Erf(a2_j)):  the terms' errors + n u sum |term| for the float32 sum;  T = exp(E): T (expm1(dE) + EXP_REL)

EXP_REL = 2.5e-7 and ERF_ABS = 5e-7 are what test_gpu_parity.py::test_device_erf_exp_against_reference_tables holds the device's accurate
Exp (relative) and its A&S / libm Erf (absolute) to; test_oracle.py holds the oracle's to less.  Results below FLT_MIN = 2^-126 may be
flushed to 0 or rounded as subnormals: TINY per operation, absolute, next to every relative error.

  density D = sum mag exp(-|p - mu|^2 / (2 sigma^2)): no cancellation, d(x) <= 8 u x, the float32 sum n u sum |term|.
  step sum: t runs through the float32 sequence 0, fl(0 + delta), fl(fl(0 + delta) + delta), ... while t <= s (`step_times`); the
    terms delta mag exp(-|o + d t - mu|^2 / (2 sigma^2)) are summed in float64; T = the oracle's fast_exp(-sum).  Bound: the terms'
    relative errors, N u sum |term| for the float32 accumulation of N = steps * n terms, times the Lipschitz factor of fast_exp (it is
    piecewise linear with slope 2^e / ln 2 <= y / ln 2 inside the binade of its result y), plus two quanta of its float32 argument
    a x + b (|a x + b| < 2^31: 128 integer steps of the mantissa each).
  radiance (rt.h:146-164): L = sum_i albedo_i sum_{k=-4..0} pdf_i(o + d s_ik) T(s_ik) sigma_i, s_ik = mubar_i + k sigma_i, with T's bound
    at s_ik (d(s) = d(mubar_i) + u (4 sigma_i + |s|)) and the density's at the sample point.

For the pairs whose Erf or Exp jumps (ERF_JUMPS, EXP_JUMPS: spline_erf_mirror by 2 * 0.0537 at 0, taylor_erf at |x| = 2, the splines at
their piece borders) `T_tolerance` and `radiance_tolerance` list the samples with an argument within its float32 error of a jump and
add the jump times the term's weight for them: the rule test_gpu_parity.py::test_alternate_approximations_render states.
"""
import functools
import math

import numpy as np

from depth_bundle_scenes import erf, erf_as, K

U = 2.0 ** -24
EXP_REL = 2.5e-7
ERF_ABS = 5e-7
TINY = 2.0 ** -126          # float32 results below it may be flushed to 0: an absolute error of up to TINY per operation
FAST_EXP_QUANTA = 2 * 128 * 2.0 ** -23
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1000)
MARKERS = {0: "magnitude 0", 1: "negative magnitude", 2: "behind the origin", 3: "centre within sigma / 10 of the ray", 4: "the origin inside"}
MARKER_FACTOR = 10.0
ACCURATE_PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1))          # (exp, erf): libm / vcl x libm / A&S
ALL_PAIRS = ACCURATE_PAIRS + ((2, 1), (3, 1), (1, 2), (1, 3), (1, 4))
# Where the reference's approximations jump, and by how much (rounded up; test_query_scenes.py::test_jump_tables measures them on the oracle):
# the cubic pieces of the splines do not meet at their borders, spline_erf_mirror is +-0.0537 either side of 0, taylor_erf 0.9721 below |x| = 2
_SPLINE_ERF_BORDERS = ((-2.3, 8.2e-4), (-1.7, 8.6e-3), (-1.1, 2.66e-2), (-0.5, 2.16e-2), (0.1, 9.09e-2), (0.7, 2.68e-2), (1.3, 8.34e-2), (1.9, 6.9e-3), (2.5, 2.22e-2),
                       (3.1, 4.3e-3))
ERF_JUMPS = {2: _SPLINE_ERF_BORDERS,
             3: ((0.0, 0.1074),) + tuple((sg * x, j) for x, j in _SPLINE_ERF_BORDERS[:4] for sg in (1, -1)) + ((-2.9, 4.2e-5), (2.9, 4.2e-5)),
             4: ((-2.0, 2.79e-2), (2.0, 2.79e-2))}
EXP_JUMPS = {3: ((-8.0, 8.4e-6), (-7.0, 6.3e-5), (-6.0, 1.37e-4), (-5.0, 4.69e-4), (-4.5, 1.02e-4), (-4.0, 1.03e-4), (-3.5, 1.94e-4), (-3.0, 3.18e-4), (-2.5, 5.04e-4),
                 (-2.0, 9.14e-4), (-1.75, 1.38e-4), (-1.5, 8.8e-5), (-1.25, 1.74e-4), (-1.0, 1.0e-4), (-0.75, 5.61e-4), (-0.5, 8.89e-4), (-0.25, 4.86e-3), (0.0, 1.62e-2))}
NRAYS = 8
ORIGIN = np.array([0.0, 0.0, -3.0])

GAUSSIAN = np.dtype([("albedo", np.float32, 4), ("mu", np.float32, 4), ("sigma", np.float32), ("magnitude", np.float32)])


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


class Scene:
    """g: the Gaussians; origins, dirs [NRAYS, 3] float32; s [NRAYS, ns] sample distances per ray; pts [npts, 3] density points"""

    def __init__(self, g, origins, dirs, s, pts):
        self.g, self.origins, self.dirs, self.s, self.pts = g, origins, dirs, s, pts
        self.n = len(g)


def reference_scene():
    """tests/transmittance.cpp:9-31 of the reference: three Gaussians, o = (0, 0, -5), d = (0, 0, 1), s = 7 + 0.75 k for k = -6 : 0.1 : 6
    (every eighth of them here), and seven more rays around that one."""
    g = np.zeros(3, GAUSSIAN)
    g["albedo"] = [[0, 1, 0, .1], [0, 0, 1, .7], [1, 0, 0, 1]]
    g["mu"][:, :3] = [[.3, .3, .5], [-.3, -.3, 0], [0, 0, 2]]
    g["sigma"], g["magnitude"] = [.1, .4, .75], [2., .7, 1.]
    rng = np.random.default_rng(3)
    origins = (rng.normal(size=(NRAYS, 3)) * 0.2 + [0, 0, -5]).astype(np.float32)
    dirs = unit(rng.normal(size=(NRAYS, 3)) * 0.06 + [0, 0, 1])
    origins[0], dirs[0] = (0, 0, -5), (0, 0, 1)
    k = np.arange(-6, 6.0001, 0.1, dtype=np.float32)[::8]
    s = np.tile((np.float32(7.0) + k * np.float32(0.75)).astype(np.float32), (NRAYS, 1))
    pts = np.concatenate([origins + dirs * s[:, 5:6], g["mu"][:, :3]]).astype(np.float32)
    return Scene(g, origins, dirs, s, pts)


@functools.lru_cache(maxsize=None)
def scene(n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    origins = (rng.normal(size=(NRAYS, 3)) * 0.15 + ORIGIN).astype(np.float32)
    dirs = unit(rng.normal(size=(NRAYS, 3)) * 0.12 + [0, 0, 1])
    origins[0], dirs[0] = ORIGIN.astype(np.float32), unit([0.05, -0.03, 1.0])
    g = np.zeros(n, GAUSSIAN)
    g["albedo"] = rng.uniform(0.05, 1.0, (n, 4))
    g["mu"][:, :3] = rng.uniform([-1, -1, -1], [1, 1, 2], (n, 3))
    g["sigma"] = rng.uniform(0.1, 0.6, n)
    # optical depth of a ray through the box stays near 2 whatever n: sum_j sigma mag sqrt(2 pi) exp(-x_j) with about a third of the
    # Gaussians within reach of a ray
    g["magnitude"] = rng.uniform(0.3, 1.0, n) * min(1.0, 12.0 / max(n, 1))
    if n >= 5:
        o, d = origins[0].astype(np.float64), dirs[0].astype(np.float64)
        side = np.cross(d, [0, 1, 0])
        side /= np.linalg.norm(side)
        g["mu"][0, :3], g["sigma"][0], g["magnitude"][0] = o + 3.0 * d + 0.1 * side, 0.3, 0.0
        g["mu"][1, :3], g["sigma"][1], g["magnitude"][1] = o + 2.5 * d - 0.1 * side, 0.35, -0.5
        g["mu"][2, :3], g["sigma"][2], g["magnitude"][2] = o - 0.8 * d + 0.05 * side, 0.4, 0.6
        g["mu"][3, :3], g["sigma"][3], g["magnitude"][3] = o + 3.6 * d + 0.02 * side, 0.25, 0.7
        g["mu"][4, :3], g["sigma"][4], g["magnitude"][4] = o + 0.2 * d + 0.1 * side, 0.5, 0.5
    far = np.linalg.norm(g["mu"][None, :, :3].astype(np.float64) - origins[:, None, :], axis=2)
    assert n == 0 or (far.max() <= 6.0 and g["sigma"].min() >= np.float32(0.1))
    assert np.abs(np.linalg.norm(dirs.astype(np.float64), axis=1) - 1).max() <= 1e-7
    s = np.tile(np.array([-1.0, 0.0, 0.5, 1.7, 2.6, 3.1, 3.7, 4.4, 6.0, 9.0], np.float32), (NRAYS, 1))
    s = (s + rng.uniform(-0.05, 0.05, s.shape) * (s != 0)).astype(np.float32)
    pts = np.concatenate([origins + dirs * s[:, 4:5], origins[:2], g["mu"][:5, :3]]).astype(np.float32)
    return Scene(g, origins, dirs, s, pts)


def all_scenes():
    return [("ref3", reference_scene())] + [(f"n{n}", scene(n)) for n in SIZES]


# ---------------------------------------------------------------------------------------------------------------------------------
class Geometry:
    """(ray, Gaussian) quantities in float64 with their float32 error bounds (module docstring).  variant: a wrong kernel, see VARIANTS"""

    def __init__(self, o, d, g, variant=None):
        f = np.float64
        self.o, self.d = np.asarray(o, np.float32).astype(f), np.asarray(d, np.float32).astype(f)
        self.mu, self.sigma, self.mag = g["mu"][:, :3].astype(f), g["sigma"].astype(f), g["magnitude"].astype(f)
        self.albedo = g["albedo"].astype(f)
        self.n = len(g)
        if variant == "abs_magnitude":
            self.mag = np.abs(self.mag)
        c = self.mu - self.o
        self.c2 = (c * c).sum(1)
        self.mubar = c @ self.d
        self.d_mubar = 4 * U * np.sqrt(self.c2) * np.linalg.norm(self.d)
        self.inv = 1.0 / (2.0 * self.sigma ** 2)
        self.x = (self.c2 - self.mubar ** 2) * self.inv
        self.d_x = 16 * U * self.c2 * self.inv + 4 * U * np.abs(self.x)
        self.r = 1.0 / (math.sqrt(2.0) * self.sigma)
        self.m = self.mubar * self.r
        self.w = self.sigma * self.mag * np.exp(-self.x) * (1.0 if variant == "no_inv_sqrt_2pi" else K)
        self.w_rel = np.expm1(self.d_x) + EXP_REL + 6 * U
        self.d_a1 = self.d_mubar * self.r + 3 * U * np.abs(self.m)


def erf_enclosed(a, e, erf_kind):
    """(Erf64(a), bound on |Erf32(a') - Erf64(a)| for |a' - a| <= e)"""
    if erf_kind == 1:
        v = erf_as(a)
        return v, np.maximum(np.abs(erf_as(a + e) - v), np.abs(erf_as(a - e) - v)) + ERF_ABS
    return erf(a), 2.0 / math.sqrt(math.pi) * np.exp(-np.maximum(0.0, np.abs(a) - e) ** 2) * e + ERF_ABS


def exponent(G, s, d_s, erf_kind, variant=None, keep=None):
    """E(s) [ns] and its bound, over the Gaussians `keep` (default all).  s, d_s: [ns]"""
    s, d_s = np.asarray(s, np.float64).reshape(-1, 1), np.broadcast_to(np.asarray(d_s, np.float64), np.shape(s)).reshape(-1, 1)
    j = slice(None) if keep is None else keep
    w, w_rel, r, m, d_a1 = G.w[j], G.w_rel[j], G.r[j], G.m[j], G.d_a1[j]
    a2 = s * r + m if variant == "erf_plus_mubar" else s * r - m
    d_a2 = d_a1 + d_s * r + 3 * U * np.abs(s * r) + U * np.abs(a2)
    e1, d_e1 = erf_enclosed(-m, d_a1, erf_kind)
    e2, d_e2 = erf_enclosed(a2, d_a2, erf_kind)
    term = w * (e1 - e2)
    d_term = np.abs(term) * w_rel + np.abs(w) * (d_e1 + d_e2 + U * np.abs(e1 - e2)) * (1 + w_rel) + 4 * TINY * (np.abs(G.sigma[j] * G.mag[j]) * K + 1)
    mass = np.abs(term).sum(1)
    return term.sum(1), d_term.sum(1) + term.shape[1] * U * mass


def T_model(o, d, s, g, erf_kind=0, variant=None):
    """T at the distances s [ns] along one ray over the whole scene: (T, bound), float64"""
    G = Geometry(o, d, g, variant)
    keep = slice(0, max(G.n - 1, 0)) if variant == "last_absorber_dropped" else None
    E, d_E = exponent(G, s, 0.0, erf_kind, variant, keep)
    T = np.exp(E)
    return T, T * (np.expm1(d_E) + EXP_REL)


def density_model(pts, g, variant=None):
    f = np.float64
    p = np.asarray(pts, np.float32).astype(f).reshape(-1, 1, 3)
    mu, sigma, mag = g["mu"][:, :3].astype(f), g["sigma"].astype(f), g["magnitude"].astype(f)
    dd = ((p - mu) ** 2).sum(2)
    x = dd / (2.0 * (sigma if variant == "density_sigma" else sigma ** 2))
    term = mag * np.exp(-x)
    mass = np.abs(term).sum(1)
    return term.sum(1), (np.abs(term) * (np.expm1(8 * U * x) + EXP_REL + U) + 2 * TINY * (np.abs(mag) + 1)).sum(1) + len(g) * U * mass


def point_terms(G, t, d_t, scale):
    """scale_j exp(-|o + d t - mu_j|^2 / (2 sigma_j^2)) for the distances t [nt] (their errors d_t): ([nt, n] terms, their relative error bounds, the exponents)"""
    t, d_t = np.asarray(t, np.float64).reshape(-1, 1, 1), np.broadcast_to(np.asarray(d_t, np.float64), np.shape(t)).reshape(-1, 1, 1)
    p = G.o + G.d * t - G.mu                                                  # [nt, n, 3]
    d_p = U * (np.abs(G.d * t) + np.abs(G.o + G.d * t) + np.abs(p)) + np.abs(G.d) * d_t
    dd = (p * p).sum(2)
    d_dd = 2 * (np.abs(p) * d_p).sum(2) + 5 * U * dd
    x = dd * G.inv
    return scale * np.exp(-x), np.expm1(d_dd * G.inv + 4 * U * x) + EXP_REL + 4 * U, x


def step_times(s, delta, variant=None):
    """the float32 sequence of t the loop `for (t = 0; t <= s; t += delta)` visits"""
    s, delta, t, out = np.float32(s), np.float32(delta), np.float32(0.0), []
    assert delta > 0 and not (s >= np.float32(0) and (np.isinf(s) or float(s) >= float(delta) * 2.0 ** 23)), "the loop would not end"
    while (t < s) if variant == "step_strict" else (t <= s):
        out.append(t)
        t = np.float32(t + delta)
    if variant == "step_one_more" and s >= 0:
        out.append(t)
    return np.array(out, np.float64)


def step_model(oracle, o, d, s, delta, g, variant=None):
    """transmittance_step at ONE sample distance s: (T, bound, steps)"""
    G = Geometry(o, d, g)
    t = step_times(s, delta, variant)
    total = d_total = 0.0
    if len(t) and G.n:
        term, rel, _ = point_terms(G, t, 0.0, float(np.float32(delta)) * G.mag)
        mass = float(np.abs(term).sum())
        total, d_total = float(term.sum()), float((np.abs(term) * rel).sum()) + term.size * (U * mass + 2 * TINY * (float(np.abs(G.mag).max()) + 1))
    T = float(oracle.map_scalar("oracle_fast_exp", np.array([-total], np.float32))[0])
    return T, T * (d_total / math.log(2.0) * (1 + d_total) + FAST_EXP_QUANTA), len(t)


def radiance_model(o, d, g, erf_kind=0, variant=None):
    """rt.h:146-164 for one ray: (L [4], bound [4])"""
    G = Geometry(o, d, g, variant)
    n = G.n
    if n == 0:
        return np.zeros(4), np.zeros(4)
    ks = np.arange(-3, 2) if variant == "samples_shifted" else np.arange(-4, 1)
    s = G.mubar[:, None] + ks[None, :] * G.sigma[:, None]                     # [n, 5]
    d_s = G.d_mubar[:, None] + U * (4 * G.sigma[:, None] + np.abs(s))
    keep = slice(0, n - 1) if variant == "last_absorber_dropped" else None
    E, d_E = exponent(G, s.ravel(), d_s.ravel(), erf_kind, variant, keep)
    E, d_E = E.reshape(n, 5), d_E.reshape(n, 5)
    val, d_val = np.empty((n, 5)), np.empty((n, 5))
    for i in range(n):   # pdf_i at its own five sample points
        Gi = Geometry(o, d, g[i:i + 1], variant)
        pdf, rel, x_pdf = (a[:, 0] for a in point_terms(Gi, s[i], d_s[i], Gi.sigma * Gi.mag))
        val[i] = pdf * np.exp(E[i])
        d_val[i] = np.abs(val[i]) * (rel + np.expm1(d_E[i]) + EXP_REL + U * (np.abs(E[i]) + x_pdf) + 2 * U) + 4 * TINY * (abs(Gi.sigma[0] * Gi.mag[0]) + 1)
    inner, d_inner = val.sum(1), d_val.sum(1) + 5 * U * np.abs(val).sum(1)
    weight = np.ones(n)
    tail = n % 4
    if tail and variant == "tail_emitter_dropped":
        weight[n - 1] = 0.0
    if tail and variant == "tail_duplicate_counted":
        weight[n - tail] += 4 - tail
    L = (G.albedo * (weight * inner)[:, None]).sum(0)
    mass = (np.abs(G.albedo) * np.abs(inner)[:, None]).sum(0)
    return L, (np.abs(G.albedo) * d_inner[:, None]).sum(0) + (n + 1) * U * mass


VARIANTS = {   # a wrong kernel: the query it breaks
    "step_strict": "step", "step_one_more": "step", "erf_plus_mubar": "T", "no_inv_sqrt_2pi": "T", "samples_shifted": "radiance",
    "tail_emitter_dropped": "radiance", "tail_duplicate_counted": "radiance", "last_absorber_dropped": "T", "abs_magnitude": "T",
    "density_sigma": "density",
}

# the step sum's cases: (delta, how far the sample points reach in steps); at most 2000 steps
STEP_CASES = ((0.25, 24), (0.01, 600))


def step_samples(delta, reach):
    """sample points for the step sum: 0, negative, NaN, exactly on steps of the float32 sequence, one ulp below and above such steps, and in between"""
    t = step_times(np.float32(delta) * np.float32(reach), delta)
    on = np.array([t[1], t[reach // 3], t[reach - 1]], np.float32)
    between = np.array([0.4 * delta, t[reach // 2] + 0.5 * delta], np.float32)
    return np.concatenate([[np.float32(0.0), np.float32(-0.5), np.float32(np.nan)], on, np.nextafter(on, np.float32(-np.inf)),
                           np.nextafter(on, np.float32(np.inf)), between]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# What both suites check, computed once per process
def model_rays(sc):
    """the rays whose radiance the models and the oracle compute: all of them, two of the 1000-Gaussian scene (5 n^2 terms per ray)"""
    return range(NRAYS if sc.n < 1000 else 2)


@functools.lru_cache(maxsize=None)
def named_scene(name):
    return reference_scene() if name == "ref3" else scene(int(name[1:]))


SCENE_NAMES = ("ref3",) + tuple(f"n{n}" for n in SIZES)


@functools.lru_cache(maxsize=None)
def models(name, erf_kind):
    """dict of float64 arrays: T, dT [NRAYS, ns]; L, dL [model rays, 4]; D, dD [npts]"""
    sc = named_scene(name)
    T, dT = zip(*(T_model(sc.origins[r], sc.dirs[r], sc.s[r], sc.g, erf_kind) for r in range(NRAYS)))
    L, dL = zip(*(radiance_model(sc.origins[r], sc.dirs[r], sc.g, erf_kind) for r in model_rays(sc)))
    D, dD = density_model(sc.pts, sc.g)
    return dict(T=np.array(T), dT=np.array(dT), L=np.array(L), dL=np.array(dL), D=D, dD=dD)


# The guard of vrt_hip_transmittance_step (csrc/vrt_step_guard.hpp): rows (sample points, delta, Gaussians, refusal or 0).  2^-10 * 2^23 = 8192
# and float32(0.01) * 2^23 = 83886.0779...; 1024 steps over 8192 Gaussians are the work cap of 2^23 exactly.
GUARD_TABLE = (
    ("1.0", "0.01", 3, 0), ("0", "0.01", 3, 0), ("-1", "0.01", 3, 0), ("nan", "0.01", 3, 0), ("-inf", "0.25", 3, 0), ("-", "0.01", 3, 0),
    ("nan,-1,0.5,0.25", "0.25", 0, 0), ("11.5,3", "0.01", 65, 0), ("500", "0.25", 65, 0),
    ("0x1.fffffep+12", "0x1p-10", 1, 0), ("8192", "0x1p-10", 1, 3), ("1,8192.001,2", "0x1p-10", 1, 3),
    ("83886.07", "0.01", 1, 0), ("83886.08", "0.01", 1, 3), ("3e5", "0.01", 1, 3), ("3e38", "1e32", 1, 0), ("3e38", "1e-3", 1, 3),
    ("inf", "0.01", 3, 2), ("1.0,inf", "0.25", 0, 2), ("inf", "1e30", 1, 2),
    ("64", "0x1p-4", 8192, 0), ("64", "0x1p-4", 8193, 4), ("64.001", "0x1p-4", 8192, 4), ("5e4", "0.01", 65, 4),
    ("0x1p22", "1", 2, 0), ("0x1p22", "1", 3, 4), ("0x1.000002p22", "1", 2, 4),
    ("1", "1e-40", 3, 1), ("0", "1e-40", 3, 1), ("1", "0", 3, 1), ("1", "-0.01", 3, 1), ("1", "nan", 3, 1),
)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU against the oracle under one (Exp, Erf) pair: the project's constants for the full sums, plus what the pair's number format adds
TOL_T = 2e-6                 # test_gpu_parity.py: T of the full sums against the oracle
TOL_RADIANCE = 2e-5          # test_gpu_parity.TOL_NOCULL: "same sum, different association / 1-ulp rcp, exp"
FAST_EXP_QUANTUM = 128 * 2.0 ** -23     # fast_exp reads its result off the float32 a x + b, |a x + b| < 2^31: arguments one ulp apart give results this far apart (relative)


def near(a, d_a, jumps):
    """the jumps (a list of (where, how much)) that lie within d_a of the argument a, added up"""
    out = np.zeros(np.broadcast(a, d_a).shape)
    for x0, j in jumps:
        out += j * (np.abs(a - x0) <= d_a)
    return out


def _sensitivity(G, s, d_s, pair):
    """per sample: (E, what a jump of the Erf may add to E, what a jump of the Exp may add to a weight's share of E, sum |term|).  The GPU and
    the oracle each carry the float32 error of an argument, so they may be twice that apart."""
    ek, rk = pair
    sv, dv = np.asarray(s, np.float64).reshape(-1, 1), np.broadcast_to(np.asarray(d_s, np.float64), np.shape(s)).reshape(-1, 1)
    a2 = sv * G.r - G.m
    d_a2 = G.d_a1 + dv * G.r + 3 * U * np.abs(sv * G.r) + U * np.abs(a2)
    delta = erf(-G.m) - erf(a2)
    mass = np.abs(G.w * delta).sum(1)
    J = np.zeros(sv.shape[0])
    if rk in ERF_JUMPS:
        J = J + (np.abs(G.w) * near(-G.m, 2 * G.d_a1, ERF_JUMPS[rk])).sum() + (np.abs(G.w) * near(a2, 2 * d_a2, ERF_JUMPS[rk])).sum(1)
    if ek in EXP_JUMPS:
        J = J + (np.abs(G.sigma * G.mag) * K * near(-G.x, 2 * G.d_x, EXP_JUMPS[ek]) * np.abs(delta)).sum(1)
    return J, mass


def T_tolerance(o, d, s, g, pair):
    """[ns]: TOL_T, and for samples the pair's format makes sensitive, the derived extra: an Erf argument, the exponent or a weight's exponent
    within its float32 error of a jump of the pair's Erf / Exp; under fast_exp one quantum for the result and one per weight."""
    ek, rk = pair
    G = Geometry(o, d, g)
    E, d_E = exponent(G, s, 0.0, 0)
    T = np.exp(E) * 1.05
    J, mass = _sensitivity(G, s, 0.0, pair)
    tol = TOL_T + T * np.expm1(J)
    if ek == 2:
        tol = tol + T * FAST_EXP_QUANTUM * (1 + mass)
    if ek in EXP_JUMPS:
        tol = tol + near(E, 2 * (d_E + J), EXP_JUMPS[ek])
    return tol


def radiance_tolerance(o, d, g, pair):
    """[4]: TOL_RADIANCE and the same extras per sample (i, k), weighted with the sample's |albedo_i pdf_i T sigma_i| -- under fast_exp three
    quanta, for the emission's two calls (emission_term) and T's weights; under spline_exp the emission's own exponent as well."""
    ek, rk = pair
    if len(g) == 0:
        return np.full(4, TOL_RADIANCE)
    G = Geometry(o, d, g)
    s = G.mubar[:, None] + np.arange(-4, 1)[None, :] * G.sigma[:, None]
    d_s = G.d_mubar[:, None] + U * (4 * G.sigma[:, None] + np.abs(s))
    E, d_E = exponent(G, s.ravel(), d_s.ravel(), 0)
    J, mass = _sensitivity(G, s.ravel(), d_s.ravel(), pair)
    E, d_E, J, mass = (a.reshape(-1, 5) for a in (E, d_E, J, mass))
    q = np.abs(G.sigma * G.mag)[:, None]
    x_pdf, d_x_pdf = np.empty_like(s), np.empty_like(s)
    for i in range(G.n):
        _, rel, x = (a[:, 0] for a in point_terms(Geometry(o, d, g[i:i + 1]), s[i], d_s[i], 1.0))
        x_pdf[i], d_x_pdf[i] = x, np.log1p(rel)
    pdf, T = np.exp(-x_pdf) * 1.05, np.exp(E) * 1.05
    extra = q * pdf * T * np.expm1(J)
    if ek == 2:
        extra += q * pdf * T * FAST_EXP_QUANTUM * (3 + mass)
    if ek in EXP_JUMPS:
        extra += q * (near(-x_pdf, 2 * d_x_pdf, EXP_JUMPS[ek]) * T + pdf * near(E, 2 * (d_E + J), EXP_JUMPS[ek]))
    return TOL_RADIANCE + (np.abs(G.albedo) * extra.sum(1)[:, None]).sum(0)
