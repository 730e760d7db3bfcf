"""Scenes, samples and tolerances for the transmittance bundles (vrt_hip_transmittance_bundle*, csrc/vrt_ray_trans_kernel.hip):
tests/test_gpu_transmittance_bundles.py runs them on the GPU, tests/test_transmittance_bundle_scenes.py checks with the oracle alone
that they test what they claim.  The scenes and rays are those of ray_bundle_scenes.py: the bundles share the radiance bundles' cull.

A ray drops Gaussian j iff sigma_j mag_j exp(-x) < eps_eff = cull_eps min(1, 4096 / N) (`kept`).  Its term of the exponent is
sigma cbar / sqrt(2 pi) (Erf(..) - Erf(..)), at most 2 / sqrt(2 pi) = 0.8 times that, so the exponent moves by less than
0.8 cull_eps min(N, 4096) -- and so does T where T <= 1 (s >= 0).
"""
import numpy as np

from ray_bundle_scenes import (RAY_PL, RAY_LCAP, CULL_EPS, TOL, kept, kept_range, coherent_rays, scattered_rays, stack, stack_rays,  # noqa: F401
                               stack_with_side, one_over_pair, wide_stack, wide_rays, normalise)

SG = 4                       # RAY_SG of csrc/vrt_ray_trans_kernel.hip: samples carried through one walk of a list
TOL_FULL_SUM = 2e-6          # what test_gpu_parity.py::test_broadcast_transmittance_rays grants the full sum against the oracle
STACK_S = np.array([0.0, 4.2, 5.0, 5.8, 6.5], np.float32)    # before, inside (three) and behind the stacks of ray_bundle_scenes.stack
WIDE_S = np.array([3.0, 5.0, 8.0], np.float32)               # before, inside and behind the wide stack
PROFILE_S = np.linspace(0.0, 8.0, 9).astype(np.float32)      # across the grid scenes from the bundles' origins


def cull_bound(n, cull_eps=CULL_EPS):
    """What the cull can move a ray's exponent by (and T, where T <= 1)."""
    return 0.8 * cull_eps * min(n, 4096)


def tolerance(lo, hi, n, cull_eps=CULL_EPS):
    """Per ray, from kept_range's (lo, hi): a ray the lane = ray kernel sums for certain (hi <= RAY_PL) is the reference's sum without
    what the cull dropped; the one-wave-per-ray kernel sums in another order, worst case T |ln T| n 2^-24 <= 0.37 * 4096 * 6e-8 = 9e-5
    -- also allowed to the rare ray whose float32 list length may fall on either side of RAY_PL."""
    return np.where(np.asarray(hi) <= RAY_PL, TOL_FULL_SUM + cull_bound(n, cull_eps), TOL)


def oracle_T(oracle, origins, dirs, s, g, exp_kind=1, erf_kind=1, rays=None, keep=None):
    """oracle.transmittance per ray over the WHOLE scene (or over the rows keep[r] of it), with the float32 origins, directions and
    samples the GPU gets.  s: [ns] shared or [rays, ns].  [len(rays), ns] float32."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    s = np.asarray(s, np.float32)
    rays = range(len(d)) if rays is None else rays
    return np.stack([oracle.transmittance(o[r if len(o) > 1 else 0], d[r], s[r] if s.ndim == 2 else s,
                                          g if keep is None else g[keep[r]], exp_kind, erf_kind) for r in rays])
