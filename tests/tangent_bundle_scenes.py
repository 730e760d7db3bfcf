"""Scenes, directions and the model for the tangent bundles (vrt_hip_radiance_rays_tangent*, csrc/vrt_ray_tangent_kernel.hip): J . v of
the radiance of any rays, forward mode.  tests/test_gpu_tangent_bundles.py runs them on the GPU, tests/test_tangent_bundle_scenes.py
checks on the CPU that the model is the derivative it claims to be, that the bound is what this file says, and that the scenes and
directions tell a wrong kernel from a right one.

Scenes, kept lists, Exp / Erf pairs and cull_eps are grad_bundle_scenes' (G); the ray part is ray_grad_rays_scenes' (RR).

The model needs no derivation of its own: the function is the one the gradient bundles differentiate, and for ray r and channel ch
G.ray_grad(..., g4 = e_ch) IS row ch of the Jacobian over the ray's kept list (`val`, with `S` the sum of the absolute values of the
addends of every entry), RR.rows_of the same row's part in the ray.  For a direction (v [N, 9] in the table's columns 0..8, rv
[nrays, 6] = d origin, d direction):
    value[r, ch] = sum val . v + row . rv,        S_T[r, ch] = sum S |v| + S_row |rv|
The bound of a component is B = RHO_T * max(S_T, S_FLOOR).  Of rv's d direction only the part perpendicular to the ray counts: the row
is perpendicular to the direction, so the model drops the rest by itself.

`ray_tangent` is the restatement of the kernel's forward-mode arithmetic (include/vrt_hip.h, "tangent bundles": three scalars per kept
Gaussian -- dmubar, u, ds --, then one pass over the pairs with the exponent and its tangent side by side), for a stack of directions
at once.  In float64 it must agree with the model (the adjoint identity, test_tangent_bundle_scenes.py); in float32, with the oracle's
Exp / Erf of the pair for the forward quantities, it measures RHO_T.

RHO_T.  The worst |t32 - t64| / S_T over every scene of G.suite with every ray, every direction of `directions`, both pairs and both
cull_eps is the float32 rounding of the formulas themselves; RHO_T is 4 times that, for another summation order, fma contraction, the
wave's order of summation and the device's exp against numpy's.  test_tangent_bundle_scenes.py::test_rho_t holds the measurement
against the constant.
"""
import numpy as np

import grad_bundle_scenes as G
import ray_grad_rays_scenes as RR
from grad_bundle_scenes import EPS, PAIRS, RAY_LCAP, RAY_PL, S_FLOOR, oracle_fns, params64, suite  # noqa: F401

K, CE, SQRT2 = G.K, G.CE, G.SQRT2
# measured on the CPU (test_rho_t prints it): worst |t32 - t64| / S_T = 6.99e-6 (vcl, A&S) and 8.30e-6 (libm, libm), both on the
# scattered grid bundle (as RHO's worst, 6.45e-6: sigma = 1 / 32 there, and x = (s - mubar) r carries ulp(|c|) r of float32 rounding); the
# coherent grid bundle is at 6.8e-6 and 6.6e-6, every other scene below 5.1e-7.  4 x 8.30e-6 = 3.32e-5.
RHO_T = 3.4e-5
VARIANTS = ("no_ds_in_dx", "no_cn_in_dmubar", "radial_counted", "e1_sign", "no_self_absorber", "no_k_term", "no_last", "do_sign",
            "no_dd2", "no_F")


def bound(S):
    return RHO_T * np.maximum(S, S_FLOOR)


def ray_tangent(o, d, alb, mu, sig, mag, v, rv, dt=np.float64, fexp=np.exp, ferf=G.erf, variant=None):
    """One ray over one kept list (arrays of its n Gaussians in list order) along nd directions at once: v [nd, n, 9] (the table's
    columns 0..8 of the kept Gaussians), rv [nd, 6] (d origin, d direction of this ray).  Returns [nd, 4] in dt.
    dt, fexp, ferf: the number format and the Exp / Erf of the forward quantities; e1 and e2 are numpy's exp in dt.
    variant: one of VARIANTS, a WRONG kernel."""
    n, nd = len(sig), len(v)
    if variant == "no_last" and n:
        return ray_tangent(o, d, alb[:-1], mu[:-1], sig[:-1], mag[:-1], v[:, :-1], rv, dt, fexp, ferf)
    mubar, cp, _ = RR.geometry(o, d, mu, dt)               # the kernels' grad_gauss: compensated c and mubar
    o, d, alb, mu, sig, mag, v, rv = (np.asarray(a, dt) for a in (o, d, alb, mu, sig, mag, v, rv))
    one = dt(1.0)
    e_mubar = ((mu - o) * d).sum(1, dtype=dt)              # where an emitter's samples sit: the plain dot product (grad_emitter_place)
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
    kk = np.arange(-4, 1).astype(dt)
    # ---- the ray's tangent, and per kept Gaussian the three scalars ----
    do, t = rv[:, :3], rv[:, 3:]
    da, dmu, dsig, dm = v[:, :, 0:4], v[:, :, 4:7], v[:, :, 7], v[:, :, 8]
    dc = dmu + do[:, None, :] if variant == "do_sign" else dmu - do[:, None, :]
    # c_perp . t: perpendicular to the ray, c_perp drops the part of t along it (the wrong kernel: c = mu - o in its place)
    cn = ((mu - o if variant == "radial_counted" else cp)[None] * t[:, None, :]).sum(2, dtype=dt)
    dmubar = (dc * d[None, None, :]).sum(2, dtype=dt)
    if variant != "no_cn_in_dmubar":
        dmubar = dmubar + cn
    dd2 = dt(2.0) * ((cp[None] * dc).sum(2, dtype=dt) - mubar[None] * cn)
    if variant == "no_dd2":
        dd2 = dd2 * dt(0.0)
    ds = dsig * inv_s[None]
    u = mag[None] * (ds - dt(0.5) * dd2 * inv_s2[None] + (d2 * inv_s2)[None] * ds) + dm
    dA = Am[None] * u
    F = ((A * dt(CE) * e1)[None] * (mr[None] * ds - dmubar * r[None])).sum(1, dtype=dt)
    if variant == "no_F":
        F = F * dt(0.0)
    out = np.zeros((nd, 4), dt)
    eb = max(1, 400000 // (5 * max(n, 1)))
    for i0 in range(0, n, eb):
        sl = slice(i0, min(n, i0 + eb))
        ne = sl.stop - sl.start
        s = e_mubar[sl, None] + kk[None, :] * sig[sl, None]
        x = (s[:, :, None] - mubar[None, None, :]) * r[None, None, :]
        D = E[None, None, :] - ferf(x)
        ACe2 = (A * dt(CE))[None, None, :] * np.exp(-(x * x))
        if variant == "no_self_absorber":
            own = np.arange(sl.start, sl.stop)[:, None, None] == np.arange(n)[None, None, :]
            D, ACe2 = np.where(own, dt(0.0), D), np.where(own, dt(0.0), ACe2)
            acc = (A[None, None, :] * (E[None, None, :] - ferf(x))).sum(2, dtype=dt)
        else:
            acc = (A[None, None, :] * D).sum(2, dtype=dt)
        tk = sig[sl, None] * fexp(acc - (d2 * inv2s2)[sl, None] - (kk * kk / dt(2.0))[None, :])       # sigma_i (pdf / m_i) T_ik
        V = tk.sum(1, dtype=dt)
        db = max(1, 1600000 // (5 * n * ne))
        for q0 in range(0, nd, db):
            qs = slice(q0, min(nd, q0 + db))
            de = dmubar[qs, sl, None] if variant == "no_k_term" else dmubar[qs, sl, None] + kk[None, None, :] * dsig[qs, sl, None]
            dx = (de[:, :, :, None] - dmubar[qs, None, None, :]) * r[None, None, None, :]
            if variant != "no_ds_in_dx":
                dx = dx - x[None] * ds[qs, None, None, :]
            dacc = (dA[qs, None, None, :] * D[None] - ACe2[None] * dx).sum(3, dtype=dt) + F[qs, None, None]
            TD = (tk[None] * dacc).sum(2, dtype=dt)
            Z = u[qs, sl] * V[None] + mag[None, sl] * TD
            out[qs] += (da[qs, sl, :] * (mag[sl] * V)[None, :, None]).sum(1, dtype=dt) + (alb[None, sl, :] * Z[:, :, None]).sum(1, dtype=dt)
    return out


# ---- directions: seeded per scene ----
def _f32(a):
    return np.asarray(a, np.float32)


def directions(sc):
    """[(name, v [N, 9] float32 or None, rv [nrays, 6] float32 or None)]: a dense random direction in every column of every Gaussian with
    ray tangents that have a component along the ray (which must not count); one-hot directions on each marker Gaussian's nine columns;
    albedo only, Gaussians only, rays only; with a shared origin, that origin alone."""
    N, nrays = len(sc.g), len(sc.d)
    rng = np.random.default_rng(9100 + sum(map(ord, sc.name)))
    dense_v = _f32(rng.uniform(-1.0, 1.0, size=(N, 9)))
    dense_rv = _f32(rng.uniform(-1.0, 1.0, size=(nrays, 6)))
    dense_rv[:, 3:] += 2.0 * sc.d                                       # along the ray: must not count
    out = [("dense", dense_v, dense_rv)]
    for j in sc.markers:
        for c in range(9):
            v = np.zeros((N, 9), np.float32)
            v[j, c] = 1.0
            out.append((f"one-hot {int(j)} {c}", v, None))
    alb = np.zeros((N, 9), np.float32)
    alb[:, :4] = rng.uniform(-1.0, 1.0, size=(N, 4))
    out += [("albedo", alb, None), ("gaussians", _f32(rng.uniform(-1.0, 1.0, size=(N, 9))), None),
            ("rays", None, _f32(rng.uniform(-1.0, 1.0, size=(nrays, 6))))]
    if sc.o.size == 3:
        shared = np.zeros((nrays, 6), np.float32)
        shared[:, :3] = _f32(rng.uniform(-1.0, 1.0, size=3))[None, :]
        out.append(("origin shared", None, shared))
    return out


def stacked(sc, dirs=None):
    """(names, v [nd, N, 9], rv [nd, nrays, 6]) float32 of the scene's directions, None as zeros"""
    dirs = directions(sc) if dirs is None else dirs
    N, nrays = len(sc.g), len(sc.d)
    v = np.stack([np.zeros((N, 9), np.float32) if a is None else a for _, a, _ in dirs])
    rv = np.stack([np.zeros((nrays, 6), np.float32) if b is None else b for _, _, b in dirs])
    return [name for name, _, _ in dirs], v, rv


# ---- the model over a bundle ----
_JAC = {}


def jacobian(sc, pair, cull_eps=1e-9):
    """Per ray (idx, Jg [4, n, 9], Sg [4, n, 9], Jr [4, 6], Sr [4, 6]) in float64: G.ray_grad and RR.rows_of with g4 = e_ch.  Computed once."""
    key = (sc.name, pair, cull_eps)
    if key not in _JAC:
        ek, fk = PAIRS[pair]
        ferf = G.erf_as if fk == 1 else G.erf
        out = []
        for r, idx in enumerate(sc.lists(cull_eps, ek)):
            n = len(idx)
            Jg, Sg, Jr, Sr = np.zeros((4, n, 9)), np.zeros((4, n, 9)), np.zeros((4, 6)), np.zeros((4, 6))
            if n:
                alb, mu, sig, mag = G.g_rows64(sc.g, idx)
                for ch in range(4):
                    Jg[ch], Sg[ch], _ = G.ray_grad(sc.origin(r), sc.d[r], alb, mu, sig, mag, np.eye(4)[ch], ferf=ferf)
                    Jr[ch], Sr[ch] = RR.rows_of(sc.origin(r), sc.d[r], mu, sig, mag, Jg[ch][:, 4:7], Sg[ch][:, 4:7], Jg[ch][:, 8], Sg[ch][:, 8])
            out.append((idx, Jg, Sg, Jr, Sr))
        _JAC[key] = out
    return _JAC[key]


def model(sc, pair, cull_eps, v, rv):
    """(value [nd, nrays, 4], S_T [nd, nrays, 4]) in float64 of the directions v [nd, N, 9], rv [nd, nrays, 6]"""
    v, rv = np.asarray(v, np.float64), np.asarray(rv, np.float64)
    val, S = np.zeros((len(v), len(sc.d), 4)), np.zeros((len(v), len(sc.d), 4))
    for r, (idx, Jg, Sg, Jr, Sr) in enumerate(jacobian(sc, pair, cull_eps)):
        val[:, r] = np.einsum("cjk,djk->dc", Jg, v[:, idx]) + rv[:, r] @ Jr.T
        S[:, r] = np.einsum("cjk,djk->dc", Sg, np.abs(v[:, idx])) + np.abs(rv[:, r]) @ Sr.T
    return val, S


def bundle_tangent(sc, pair, cull_eps, v, rv, dt=np.float64, fexp=None, ferf=None, variant=None):
    """ray_tangent over the bundle: [nd, nrays, 4] in dt; a ray that keeps nothing: zeros"""
    ek, fk = PAIRS[pair]
    if fexp is None:
        fexp, ferf = np.exp, (G.erf_as if fk == 1 else G.erf)
    out = np.zeros((len(v), len(sc.d), 4), dt)
    for r, idx in enumerate(sc.lists(cull_eps, ek)):
        if len(idx):
            out[:, r] = ray_tangent(sc.origin(r), sc.d[r], *G.g_rows64(sc.g, idx), v[:, idx], rv[:, r], dt, fexp, ferf, variant)
    return out


def measured_ratio(oracle, sc, pair, cull_eps):
    """worst |t32 - t64| / S_T of the scene over its whole bundle and all its directions"""
    _, v, rv = stacked(sc)
    fexp, ferf = oracle_fns(oracle, pair)
    t64, S = model(sc, pair, cull_eps, v, rv)
    t32 = bundle_tangent(sc, pair, cull_eps, v, rv, np.float32, fexp, ferf)
    on = S > S_FLOOR
    return float((np.abs(t32.astype(np.float64) - t64)[on] / S[on]).max()) if on.any() else 0.0


# ---- what the library takes ----
def packed(v, N):
    """v [N, 9] (or None) as the library's tangent table float32 [N, 12], columns 9..11 zero"""
    if v is None:
        return None
    t = np.zeros((N, 12), np.float32)
    t[:, :9] = v
    return t


def packed_rays(rv, nrays):
    """rv [nrays, 6] (or None) as the library's ray tangents float32 [nrays, 8]"""
    if rv is None:
        return None
    t = np.zeros((nrays, 8), np.float32)
    t[:, 0:3], t[:, 4:7] = rv[:, :3], rv[:, 3:]
    return t
