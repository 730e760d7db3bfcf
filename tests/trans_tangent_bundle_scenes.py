"""Directions, the model and the bound for the transmittance tangent bundles (vrt_hip_transmittance_bundle_tangent*,
csrc/vrt_ray_trans_tangent_kernel.hip): J . v of the transmittance at sample distances along any rays and, in depth mode, of the depth at
which it falls to a level, forward mode.  tests/test_gpu_trans_tangent_bundles.py runs them on the GPU,
tests/test_trans_tangent_bundle_scenes.py checks on the CPU that the model is the derivative it claims to be, that the bound is what this
file says, and that the cases and directions tell a wrong kernel from a right one.

Cases (scenes, samples, levels, kept lists, Exp / Erf pairs, cull_eps) are trans_grad_bundle_scenes' (T), exactly; the ray part is
ray_grad_rays_scenes' (RR).

The model needs no derivation of its own: the function is the one the transmittance gradient bundles differentiate, and for ray r and
sample k T.ray_tgrad(..., g = e_k) IS row (r, k) of the Jacobian over the ray's kept list (`val` over the table's columns 4..8 with `S`
the sum of the absolute values of the addends of every entry; `gs`, `Sgs` the entry in the sample or level), RR.rows_of the same row's
part in the ray.  For a direction (v [N, 5] in the table's columns 4..8, rv [nrays, 6] = d origin, d direction, sd [nrays, ns] = d s in T
mode, d tau in depth mode):
    value[r, k] = sum val . v + row . rv[r] + gs sd[r, k],        S_T[r, k] = sum S |v| + S_row |rv[r]| + Sgs |sd[r, k]|
The bound of a component is B = RHO_TT * max(S_T, S_FLOOR).  A depth-mode sample whose depth is +inf, 0 or NaN has value 0 and S_T 0.

`ray_ttangent` is the restatement of the kernel's forward-mode arithmetic (include/vrt_hip.h, "transmittance tangent bundles": the
tangent bundles' three scalars per kept Gaussian -- dmubar, u, ds --, then one walk with E_k, S_k and dE_k side by side), for a stack of
directions at once.  In float64 it must agree with the model (the adjoint identity); in float32, with the oracle's Exp / Erf of the pair
for the forward quantities, it measures RHO_TT.

RHO_TT.  The worst |t32 - t64| / S_T over every case of T.cases (both modes, every ray and sample) with every direction of `directions`,
both pairs and both cull_eps is the float32 rounding of the formulas themselves; RHO_TT is 4 times that, the project's margin for another
summation order, fma contraction, the wave's order of summation and the device's exp against numpy's.
test_trans_tangent_bundle_scenes.py::test_rho_tt holds the measurement against the constant.
"""
import numpy as np

import grad_bundle_scenes as G
import ray_grad_rays_scenes as RR
import trans_grad_bundle_scenes as T
from grad_bundle_scenes import CE, EPS, K, PAIRS, RAY_LCAP, RAY_PL, S_FLOOR, SQRT2, oracle_fns  # noqa: F401
from trans_grad_bundle_scenes import SG, TGRAD_DEPTH, TGRAD_T, case, cases  # noqa: F401

# measured on the CPU (test_rho_tt prints it): worst |t32 - t64| / S_T = 1.887e-5 (vcl, A&S) and 1.898e-5 (libm, libm), both on "T grid16
# scattered" along the per-ray sample direction: the entry T_k S_k ds_k, which is the reverse model's grad_s and its RHO_T's worst (1.90e-5)
# for the same reason -- the grid's sigma is 1 / 32, x = (s - mubar) r carries ulp(mubar) r of float32 rounding, and e2 = exp(-x^2) of a
# sample four sigma and more from a Gaussian passes it on as 2 |x| dx.  "T grid16 coherent": 1.49e-5 (shared samples); depth mode's worst
# is 1.09e-5 ("depth grid16 coherent", one-hot on a marker's d mu y), "depth grid16 scattered" 7.8e-6; every other case is below 3.4e-6.
# 4 x 1.898e-5 = 7.6e-5.
RHO_TT = 7.6e-5
VARIANTS = ("no_sdot", "sdot_sign", "no_F", "e1_sign", "no_x_ds", "c_not_perp", "depth_sign", "depth_TS", "tau_not_over_T", "no_last_entry",
            "no_last_sample", "do_sign")
NCOL = T.NCOL


def bound(S):
    return RHO_TT * np.maximum(S, S_FLOOR)


def ray_ttangent(o, d, mu, sig, mag, s, v, rv, sd, wrt, dt=np.float64, fexp=np.exp, ferf=G.erf, variant=None):
    """One ray over one kept list (arrays of its n Gaussians in list order) at ns samples s along nd directions at once: v [nd, n, 5] (the
    table's columns 4..8 of the kept Gaussians), rv [nd, 6] (d origin, d direction of this ray), sd [nd, ns] (d s, or d tau).  Returns
    [nd, ns] in dt.  dt, fexp, ferf: the number format and the Exp / Erf of the forward quantities; e1 and e2 are numpy's exp in dt.
    variant: one of VARIANTS, a WRONG kernel."""
    n, nd = len(sig), len(v)
    if variant == "no_last_entry" and n:
        return ray_ttangent(o, d, mu[:-1], sig[:-1], mag[:-1], s, v[:, :-1], rv, sd, wrt, dt, fexp, ferf)
    mubar, cp, _ = RR.geometry(o, d, mu, dt)               # the kernels' grad_gauss: compensated c and mubar
    o, d, mu, sig, mag, s, v, rv, sd = (np.asarray(a, dt) for a in (o, d, mu, sig, mag, s, v, rv, sd))
    one = dt(1.0)
    d2 = (cp * cp).sum(1)
    inv_s = one / sig
    r = inv_s / dt(SQRT2)
    inv_s2 = inv_s * inv_s
    inv2s2 = one / (dt(2.0) * sig * sig)
    Am = dt(K) * sig * fexp(-(d2 * inv2s2))
    A = Am * mag
    mr = mubar * r
    E = ferf(-mr)
    e1 = np.exp(-(mr * mr))
    if variant == "e1_sign":
        e1 = -e1
    # ---- the ray's tangent, and per kept Gaussian the three scalars (tangent_gauss) ----
    do, t = rv[:, :3], rv[:, 3:]
    dmu, dsig, dm = v[:, :, 0:3], v[:, :, 3], v[:, :, 4]
    dc = dmu + do[:, None, :] if variant == "do_sign" else dmu - do[:, None, :]
    cn = ((mu - o if variant == "c_not_perp" else cp)[None] * t[:, None, :]).sum(2, dtype=dt)
    dmubar = (dc * d[None, None, :]).sum(2, dtype=dt) + cn
    dd2 = dt(2.0) * ((cp[None] * dc).sum(2, dtype=dt) - mubar[None] * cn)
    ds = dsig * inv_s[None]
    u = mag[None] * (ds - dt(0.5) * dd2 * inv_s2[None] + (d2 * inv_s2)[None] * ds) + dm
    dA = Am[None] * u
    F = ((A * dt(CE) * e1)[None] * (mr[None] * ds - dmubar * r[None])).sum(1, dtype=dt)          # [nd]
    if variant == "no_F":
        F = F * dt(0.0)
    # ---- the samples: E_k, S_k and dE_k side by side ----
    live = np.ones(len(s), bool)
    if wrt == TGRAD_DEPTH:
        live = np.isfinite(s) & (s > 0)
    sv = np.where(live, s, dt(0.0))
    x = (sv[:, None] - mubar[None, :]) * r[None, :]        # [ns, n], the difference first (trans_grad_x)
    D = E[None, :] - ferf(x)
    e2 = np.exp(-(x * x))
    Tk = fexp((A[None, :] * D).sum(1, dtype=dt))
    Sk = (-(A * dt(CE) * r)[None, :] * e2).sum(1, dtype=dt)
    ACe2 = (A * dt(CE))[None, :] * e2
    dxs = (dmubar * r[None])[:, None, :]
    if variant != "no_x_ds":
        dxs = dxs + x[None] * ds[:, None, :]
    dE = (dA[:, None, :] * D[None] + ACe2[None] * dxs).sum(2, dtype=dt) + F[:, None]               # [nd, ns]
    if variant == "no_sdot":
        sd = sd * dt(0.0)
    if variant == "sdot_sign":
        sd = -sd
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if wrt == TGRAD_DEPTH:
            ok = live & (Sk != 0)
            lead = sd if variant == "tau_not_over_T" else sd / Tk[None]
            num = lead + dE if variant == "depth_sign" else lead - dE
            out = np.where(ok[None], num / ((Tk * Sk) if variant == "depth_TS" else Sk)[None], dt(0.0))
        else:
            out = Tk[None] * (dE + Sk[None] * sd)
    if variant == "no_last_sample" and out.shape[1]:
        out = out.copy()
        out[:, -1] = 0
    return out.astype(dt)


# ---- directions: seeded per case ----
def _f32(a):
    return np.asarray(a, np.float32)


def directions(c):
    """[(name, v [N, 5] float32 or None, rv [nrays, 6] float32 or None, sd [nrays, ns] / [ns] float32 or None)] of case c: a dense random
    direction in columns 4..8 of every Gaussian with ray tangents that have a component of 2 along the ray (which must not count) and
    dense sample tangents; one-hot directions on each marker Gaussian's five columns; Gaussians only, rays only, samples only (per ray,
    and shared by the rays); with a shared origin, that origin alone."""
    sc = c.sc
    N, nrays, ns = len(sc.g), len(sc.d), c.ns
    rng = np.random.default_rng(7300 + sum(map(ord, c.name)))
    dense_rv = _f32(rng.uniform(-1.0, 1.0, size=(nrays, 6)))
    dense_rv[:, 3:] += 2.0 * sc.d                                       # along the ray: must not count
    out = [("dense", _f32(rng.uniform(-1.0, 1.0, size=(N, NCOL))), dense_rv, _f32(rng.uniform(-1.0, 1.0, size=(nrays, ns))))]
    for j in sc.markers:
        for col in range(NCOL):
            v = np.zeros((N, NCOL), np.float32)
            v[j, col] = 1.0
            out.append((f"one-hot {int(j)} {col}", v, None, None))
    out += [("gaussians", _f32(rng.uniform(-1.0, 1.0, size=(N, NCOL))), None, None),
            ("rays", None, _f32(rng.uniform(-1.0, 1.0, size=(nrays, 6))), None),
            ("samples", None, None, _f32(rng.uniform(-1.0, 1.0, size=(nrays, ns)))),
            ("samples shared", None, None, _f32(rng.uniform(-1.0, 1.0, size=ns)))]
    if sc.o.size == 3:
        shared = np.zeros((nrays, 6), np.float32)
        shared[:, :3] = _f32(rng.uniform(-1.0, 1.0, size=3))[None, :]
        out.append(("origin shared", None, shared, None))
    return out


def stacked(c, dirs=None):
    """(names, v [nd, N, 5], rv [nd, nrays, 6], sd [nd, nrays, ns]) float32 of the case's directions, None as zeros, shared sample
    tangents as every ray's"""
    dirs = directions(c) if dirs is None else dirs
    N, nrays, ns = len(c.sc.g), len(c.sc.d), c.ns
    v = np.stack([np.zeros((N, NCOL), np.float32) if a is None else a for _, a, _, _ in dirs])
    rv = np.stack([np.zeros((nrays, 6), np.float32) if b is None else b for _, _, b, _ in dirs])
    sd = np.stack([np.zeros((nrays, ns), np.float32) if e is None else np.broadcast_to(e, (nrays, ns)) for _, _, _, e in dirs])
    return [name for name, _, _, _ in dirs], v, rv, sd


# ---- the model over a bundle ----
_ROWS = {}


def jacobian_rows(c, erf_kind, r, idx, s):
    """Rows (r, k) of the Jacobian of case c over the list idx at the samples s [ns], float64: (Jg [ns, n, 5], Sg, Jr [ns, 6], Sr,
    Js [ns], Ss).  One T.ray_tgrad and one RR.rows_of per sample, with g = 1 at that sample alone; computed once per (ray, list, sample)."""
    sc = c.sc
    ferf = G.erf_as if erf_kind == 1 else G.erf
    n, ns = len(idx), len(s)
    Jg, Sg, Jr, Sr, Js, Ss = np.zeros((ns, n, NCOL)), np.zeros((ns, n, NCOL)), np.zeros((ns, 6)), np.zeros((ns, 6)), np.zeros(ns), np.zeros(ns)
    if not n:
        return Jg, Sg, Jr, Sr, Js, Ss
    mu, sig, mag = (np.asarray(a, np.float64) for a in T._rows(sc.g, idx))
    o, d = sc.origin(r), sc.d[r]
    head = (c.name, c.wrt, erf_kind, r, idx.tobytes())
    for k in range(ns):
        key = head + (np.float64(s[k]).tobytes(),)
        if key not in _ROWS:
            val, S, gs, Sgs, _, _ = T.ray_tgrad(o, d, mu, sig, mag, s[k:k + 1], np.ones(1), c.wrt, ferf=ferf)
            row, Srow = RR.rows_of(o, d, mu, sig, mag, val[:, 0:3], S[:, 0:3], val[:, 4], S[:, 4])
            _ROWS[key] = (val, S, row, Srow, float(gs[0]), float(Sgs[0]))
        Jg[k], Sg[k], Jr[k], Sr[k], Js[k], Ss[k] = _ROWS[key]
    return Jg, Sg, Jr, Sr, Js, Ss


def model(c, pair, cull_eps, s, v, rv, sd):
    """(value [nd, nrays, ns], S_T [nd, nrays, ns]) in float64 of the directions v [nd, N, 5], rv [nd, nrays, 6], sd [nd, nrays, ns] at
    the samples s ([ns] shared or [nrays, ns]; depth mode: the depths)"""
    ek, fk = PAIRS[pair]
    sc = c.sc
    v, rv, sd = np.asarray(v, np.float64), np.asarray(rv, np.float64), np.asarray(sd, np.float64)
    val, S = np.zeros((len(v), len(sc.d), c.ns)), np.zeros((len(v), len(sc.d), c.ns))
    for r, idx in enumerate(sc.lists(cull_eps, ek)):
        Jg, Sg, Jr, Sr, Js, Ss = jacobian_rows(c, fk, r, np.asarray(idx), np.asarray(c.samples(r, s), np.float64))
        val[:, r] = np.einsum("kjc,djc->dk", Jg, v[:, idx]) + rv[:, r] @ Jr.T + sd[:, r] * Js[None, :]
        S[:, r] = np.einsum("kjc,djc->dk", Sg, np.abs(v[:, idx])) + np.abs(rv[:, r]) @ Sr.T + np.abs(sd[:, r]) * Ss[None, :]
    return val, S


def bundle_ttangent(c, pair, cull_eps, s, v, rv, sd, dt=np.float64, fexp=None, ferf=None, variant=None):
    """ray_ttangent over the bundle: [nd, nrays, ns] in dt; a ray that keeps nothing: zeros"""
    ek, fk = PAIRS[pair]
    if fexp is None:
        fexp, ferf = np.exp, (G.erf_as if fk == 1 else G.erf)
    sc = c.sc
    out = np.zeros((len(v), len(sc.d), c.ns), dt)
    for r, idx in enumerate(sc.lists(cull_eps, ek)):
        if len(idx):
            out[:, r] = ray_ttangent(sc.origin(r), sc.d[r], *T._rows(sc.g, idx), c.samples(r, s), v[:, idx], rv[:, r], sd[:, r], c.wrt, dt, fexp, ferf,
                                     variant)
    return out


def measured_ratio(oracle, c, pair, cull_eps):
    """(worst |t32 - t64| / S_T of the case over its whole bundle and all its directions, the direction's name)"""
    names, v, rv, sd = stacked(c)
    fexp, ferf = oracle_fns(oracle, pair)
    s = T.samples_of(c, pair, cull_eps)
    t64, S = model(c, pair, cull_eps, s, v, rv, sd)
    t32 = bundle_ttangent(c, pair, cull_eps, s, v, rv, sd, np.float32, fexp, ferf)
    on = S > S_FLOOR
    if not on.any():
        return 0.0, ""
    ratio = np.where(on, np.abs(t32.astype(np.float64) - t64) / np.maximum(S, S_FLOOR), 0.0)
    j = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[j]), names[j[0]]


# ---- what the library takes ----
def packed(v, N):
    """v [N, 5] (or None) as the library's tangent table float32 [N, 12]: columns 4..8, the others zero"""
    if v is None:
        return None
    t = np.zeros((N, 12), np.float32)
    t[:, 4:9] = v
    return t


def packed_rays(rv, nrays):
    """rv [nrays, 6] (or None) as the library's ray tangents float32 [nrays, 8]"""
    if rv is None:
        return None
    t = np.zeros((nrays, 8), np.float32)
    t[:, 0:3], t[:, 4:7] = rv[:, :3], rv[:, 3:]
    return t
