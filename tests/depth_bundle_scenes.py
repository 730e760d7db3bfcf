"""Scenes, a float64 model and tolerances for the depth bundles (vrt_hip_depth_bundle*, csrc/vrt_ray_depth_kernel.hip):
tests/test_gpu_depth_bundles.py runs them on the GPU, tests/test_depth_bundle_scenes.py checks with the oracle and the model alone
that they test what they claim.  The scenes and rays are those of ray_bundle_scenes.py, the tolerance in T is the transmittance
bundles' own (transmittance_bundle_scenes.tolerance): a depth bundle inverts the very T(s) those bundles evaluate.

Model (`RayModel`), over the Gaussians a ray keeps (`kept`), in float64 with math.erf -- for the (vcl, A&S) pair with the
Abramowitz-Stegun form the reference integrates with under that pair (`erf_as`: it is up to 5e-4 off erf and moves T by 5e-6 on
the grid-16 rays, twice their tolerance) -- and with mubar_j and the exponent of cbar_j in the reference's float32 operations (see
RayModel):
    E(s) = sum_j w_j (erf(-m_j) - erf(s / (sqrt2 sigma_j) - m_j)),   w_j = sigma_j cbar_j K,   m_j = mubar_j / (sqrt2 sigma_j),
    cbar_j = mag_j exp(-(|oc_j|^2 - mubar_j^2) / (2 sigma_j^2)),   K = 1 / 0.79788456 (rt.h:18-20),   T(s) = exp(E(s)),
    T_inf = exp(sum_j w_j (erf(-m_j) - 1)),   s_end = max(0, max_j mubar_j + 6 sqrt2 sigma_j),   |dT/ds| in closed form,
    root(tau) by bisection on [0, s_end].

Acceptance of a finite result s* for the level tau (`check_finite`), tol_T the transmittance bundles' tolerance of that ray:
    delta = 4 max(ulp32(s*), s_end 2^-24)                     four times the resolution of the bracket the kernel returns
    oracle_T(s* - delta) >= tau - tol_T   and   oracle_T(s* + delta) <= tau + tol_T      (the oracle over the whole scene)
    |s* - root(tau)| <= delta + tol_T / slope   where the model's slope at its root is above 0.05
Acceptance of misses (`miss_classes`): T_inf > tau + tol_T must give +inf, T_inf < tau - tol_T must be finite, pairs in between are
excluded from the miss check -- at most 5 % of a test's (ray, level) pairs (`EXCLUDED_CAP`; the CPU suite asserts it per case list).
"""
import math

import numpy as np

from ray_bundle_scenes import (RAY_PL, RAY_LCAP, CULL_EPS, TOL, MARKER_FACTOR, kept, kept_range, coherent_rays, scattered_rays, stack,  # noqa: F401
                               stack_rays, stack_with_side, one_over_pair, wide_stack, wide_rays)
from transmittance_bundle_scenes import SG, TOL_FULL_SUM, cull_bound, tolerance, oracle_T  # noqa: F401

K = 1.0 / 0.7978845608028654
EXCLUDED_CAP = 0.05
SLOPE_MIN = 0.05
PARITY_LEVELS = np.array([0.99, 0.9, 0.5, 0.1], np.float32)
# The stacks of ray_bundle_scenes.stack have optical depth 2 along the axis (T_inf = exp(-2) = 0.135): four levels inside, the marker
# level just above T_inf, where the root sits in the last Gaussian, and a level the axial rays never reach
STACK_LEVELS = np.array([0.9, 0.75, 0.6, 0.55], np.float32)
STACK_MARKER_LEVELS = np.array([0.15, 0.17], np.float32)   # of stack_rays()' axial ray (T_inf 0.135) and the ray 0.02 off the axis (T_inf 0.158)
STACK_MISS_LEVEL = np.float32(0.1)
# the wide stack: T(5) ~ 0.42 behind most of its four markers, T_inf 0.16 .. 0.25; without one marker T_inf is at most 0.33
WIDE_LEVELS = np.array([0.9, 0.5], np.float32)
WIDE_MARKER_LEVEL = np.float32(0.35)
WIDE_MISS_LEVEL = np.float32(0.1)

_erf = np.frompyfunc(math.erf, 1, 1)


def erf(x):
    return _erf(np.asarray(x, np.float64)).astype(np.float64)


def erf_as(x):
    """Abramowitz-Stegun 7.1.27, the reference's ERF_AS (approx.cpp:90-110), in float64: up to 5e-4 off erf"""
    x = np.asarray(x, np.float64)
    t = np.abs(x)
    p = 1.0 + t * (0.278393 + t * (0.230389 + t * (0.000972 + t * 0.078108)))
    return np.copysign(1.0 - 1.0 / p ** 4, x)


ERF = {0: erf, 1: erf_as}     # by Erf kind (oracle.ERF_LIBM, ERF_AS): the function the selected pair integrates with


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


class RayModel:
    """One ray (float32 origin and direction, as the GPU gets them) over the rows `keep` of g, in float64 -- but for mubar_j and
    x_j = (|oc_j|^2 - mubar_j^2) / (2 sigma_j^2), which are the reference's float32 operations in the reference's order (rt.h:110-116):
    the difference of two numbers of size |oc|^2 ~ 25 carries a few 1e-6 of rounding noise, times 1 / (2 sigma^2) = 512 on the grid
    scenes, and the reference's T -- the oracle's, the GPU's -- is the one with that noise in it.  With x_j in float64 the model is
    1.6e-4 off the oracle on the grid-16 rays, 70 times the tolerance it is to be used with."""

    def __init__(self, o, d, g, keep=None, erf_kind=0):
        self.erf = ERF[erf_kind]
        f = np.float32
        o, d = np.asarray(o, f), np.asarray(d, f)
        g = g if keep is None else g[keep]
        sigma32, c = g["sigma"].astype(f), g["mu"][:, :3].astype(f) - o
        mubar32 = (c[:, 0] * d[0] + c[:, 1] * d[1]) + c[:, 2] * d[2]
        oc_sq = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        x32 = (oc_sq - mubar32 * mubar32) * (f(1.0) / ((f(2.0) * sigma32) * sigma32))
        sigma, mag, mubar = sigma32.astype(np.float64), g["magnitude"].astype(np.float64), mubar32.astype(np.float64)
        self.w = sigma * mag * np.exp(-x32.astype(np.float64)) * K
        self.sq = math.sqrt(2.0) * sigma
        self.m = mubar / self.sq
        self.e0 = self.erf(-self.m)
        self.s_end = max(0.0, float((mubar + 6.0 * self.sq).max())) if len(g) else 0.0
        self.T_inf = math.exp(float((self.w * (self.e0 - 1.0)).sum()))

    def T(self, s):
        return math.exp(float((self.w * (self.e0 - self.erf(s / self.sq - self.m))).sum()))

    def slope(self, s):
        """|dT/ds|, with erf's derivative (the A&S form follows erf to 5e-4: its own derivative is within a percent of this)"""
        return self.T(s) * float((self.w * (2.0 / math.sqrt(math.pi)) * np.exp(-(s / self.sq - self.m) ** 2) / self.sq).sum())

    def root(self, tau):
        """The s in (0, s_end] with T(s) = tau, or None where T(0) <= tau or T(s_end) > tau."""
        tau = float(tau)
        if not (self.T(0.0) > tau >= self.T(self.s_end)):
            return None
        lo, hi = 0.0, self.s_end
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if self.T(mid) <= tau:
                hi = mid
            else:
                lo = mid
        return hi


def models(o, d, g, rays=None, cull_eps=CULL_EPS, exp_kind=1, erf_kind=0):
    """{ray: RayModel over what the ray keeps}"""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    keep = kept(o, d, g, cull_eps, exp_kind)
    rays = range(len(d)) if rays is None else rays
    return {r: RayModel(o[r if len(o) > 1 else 0], d[r], g, keep[r], erf_kind) for r in rays}


def ray_tolerances(o, d, g, cull_eps=CULL_EPS, exp_kind=1):
    """tol_T per ray: TOL_FULL_SUM + cull_bound(n) for a ray the lane = ray kernel sums for certain, TOL for the others."""
    lo, hi = kept_range(o, d, g, cull_eps, exp_kind)
    return tolerance(lo, hi, len(g), cull_eps)


def delta_s(s_star, s_end):
    return 4.0 * max(ulp32(s_star), s_end * 2.0 ** -24)


def s_tolerance(model, tau, tol_T, s_star=None):
    """delta + tol_T / slope at the model's root (None without a root or where the slope is at most SLOPE_MIN)."""
    s64 = model.root(tau)
    if s64 is None:
        return None
    slope = model.slope(s64)
    if slope <= SLOPE_MIN:
        return None
    return delta_s(s64 if s_star is None else s_star, model.s_end) + tol_T / slope


def miss_classes(mods, levels, tol_T):
    """[len(mods), nt] int8 in the order of mods: +1 must be +inf, -1 must be finite, 0 excluded.  levels: [nt] or [rays, nt] (rows by ray id)."""
    levels = np.asarray(levels, np.float64)
    out = np.zeros((len(mods), levels.shape[-1]), np.int8)
    for i, (r, m) in enumerate(mods.items()):
        lv = levels[r] if levels.ndim == 2 else levels
        out[i] = np.where(m.T_inf > lv + tol_T[r], 1, np.where(m.T_inf < lv - tol_T[r], -1, 0))
    return out


def check_misses(depth, mods, levels, tol_T, what=""):
    """depth: [rays, nt] of the GPU, rows by ray id.  Returns the excluded share."""
    cls = miss_classes(mods, levels, tol_T)
    got = np.stack([np.asarray(depth)[r] for r in mods])
    assert np.isinf(got[cls == 1]).all() and (got[cls == 1] > 0).all(), f"{what}: a ray that stays above its level did not give +inf"
    assert np.isfinite(got[cls == -1]).all(), f"{what}: a ray that falls below its level gave no finite depth"
    excluded = float((cls == 0).mean())
    assert excluded <= EXCLUDED_CAP, (what, excluded)
    return excluded


def check_finite(oracle, o, d, g, r, s_star, tau, tol_T, model, pair=(1, 1), what=""):
    """The acceptance of one finite result (see the module's docstring).  Returns (delta, |s* - s64| or None, its bound or None)."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    s_star, tau = float(s_star), float(tau)
    delta = delta_s(s_star, model.s_end)
    around = np.array([s_star - delta, s_star + delta], np.float32)
    T = oracle.transmittance(o[r if len(o) > 1 else 0], d[r], around, g, pair[0], pair[1]).astype(np.float64)
    assert T[0] >= tau - tol_T, f"{what} ray {r} tau {tau}: oracle T({around[0]}) = {T[0]} is already below the level (s* = {s_star})"
    assert T[1] <= tau + tol_T, f"{what} ray {r} tau {tau}: oracle T({around[1]}) = {T[1]} is still above the level (s* = {s_star})"
    bound = s_tolerance(model, tau, tol_T, s_star)
    if bound is None:
        return delta, None, None
    off = abs(s_star - model.root(tau))
    assert off <= bound, f"{what} ray {r} tau {tau}: s* = {s_star}, float64 root {model.root(tau)}, bound {bound}"
    return delta, off, bound


def per_ray_levels(levels, nrays, seed=23):
    """[nrays, nt]: every ray gets the levels in an order of its own."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.permutation(levels) for _ in range(nrays)]).astype(np.float32))
