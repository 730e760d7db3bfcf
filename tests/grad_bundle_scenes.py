"""Scenes, rays and the model for the gradient bundles (vrt_hip_radiance_rays_grad*, csrc/vrt_ray_grad_kernel.hip):
tests/test_gpu_grad_bundles.py runs them on the GPU, tests/test_grad_bundle_scenes.py checks on the CPU that the model is the
derivative it claims to be, that the bound is what this file says, and that the scenes can tell a wrong kernel from a right one.

The function (include/vrt_hip.h has the contract; K = 1 / 0.79788456 is the library's constant, C = 2 / sqrt(pi)).  For one ray
(o, n) and the list it keeps (`kept`, the cull rule of tests/ray_bundle_scenes.py in float64), with c = mu - o, mubar = c.n,
c_perp = c - mubar n, d2 = |c_perp|^2, r = 1 / (sqrt2 sigma):
    A_j = K sigma_j m_j exp(-d2_j / (2 sigma_j^2)),   x_ikj = (mubar_i + k sigma_i - mubar_j) r_j,   D_ikj = erf(-mubar_j r_j) - erf(x_ikj)
    T_ik = exp(sum_j A_j D_ikj),   L = sum_i a_i sum_k sigma_i m_i exp(-d2_i / (2 sigma_i^2) - k^2 / 2) T_ik,      k = -4..0
`ray_grad` is the list of contributions ("Gradient bundles"), addend by addend, over one kept list: per output component the value and
S, the sum of the absolute values of all its addends.  The bound of a component is B = RHO * S.

RHO.  `ray_grad` runs in float32 as well, with the oracle's Exp / Erf of the pair for the forward quantities (`measured_ratio`): the worst
|g32 - g64| / S over the scenes of this file is the float32 rounding of the formulas themselves; RHO is 4 times that, for another
summation order, fma contraction, the order of the atomic adds and the device's exp against numpy's.  Every scene is measured with
every ray of its bundle.  test_grad_bundle_scenes.py::test_rho holds the measurement against the constant.
"""
import functools
import math

import numpy as np

import ray_bundle_scenes as R
from ray_bundle_scenes import RAY_PL, RAY_LCAP, EXP_FLOOR, normalise  # noqa: F401

K = 1.0 / 0.7978845608028654
CE = 2.0 / math.sqrt(math.pi)
SQRT2 = math.sqrt(2.0)
PAIRS = {"vcl-as": (1, 1), "libm-libm": (0, 0)}     # (Exp, Erf): the same numbers in the package and in the oracle
EPS = (1e-9, 0.0)                                   # the cull_eps the GPU suite runs
# measured on the CPU (test_rho prints it): worst |g32 - g64| / S = 6.45e-6 (vcl, A&S), 6.43e-6 (libm, libm), both on the scattered grid
# bundle (the grid's sigma is 1 / 32, and x = (s - mubar) r carries ulp(|c|) r of float32 rounding); the coherent grid bundle is at 1.6e-6,
# every other scene below 7e-7
RHO = 2.6e-5
COLS = {"albedo": slice(0, 4), "mu": slice(4, 7), "sigma": 7, "magnitude": 8}

try:
    from scipy.special import erf as _erf64
except ImportError:                                  # the same function, slower
    _pyerf = np.frompyfunc(math.erf, 1, 1)

    def _erf64(x):
        return _pyerf(x).astype(np.float64)


def erf(x):
    return _erf64(np.asarray(x, np.float64))


def erf_as(x):
    """Abramowitz-Stegun 7.1.27 in float64: what the A&S pair's Erf approximates to float32 rounding."""
    x = np.asarray(x, np.float64)
    t = np.abs(x)
    p = (((0.078108 * t + 0.000972) * t + 0.230389) * t + 0.278393) * t + 1.0
    return np.copysign(1.0 - 1.0 / (p * p) ** 2, x)


VARIANTS = ("no_self_absorber", "no_k_term", "no_n_term", "e1_sign", "no_d2_term", "no_k0", "no_alpha", "no_last", "no_tail",
            "double_absorber")


def ray_grad(o, d, alb, mu, sig, mag, g4, dt=np.float64, fexp=np.exp, ferf=erf, variant=None):
    """One ray over one kept list (arrays of its n Gaussians in list order).  Returns (val [n, 9], S [n, 9] float64, L [4]).
    dt, fexp, ferf: the number format and the Exp / Erf of the forward quantities (A, T, the pdf, D); e1 and e2 are numpy's exp in dt.
    variant: one of VARIANTS, a WRONG model."""
    n = len(sig)
    if variant == "no_last" and n:
        v, s, L = ray_grad(o, d, alb[:-1], mu[:-1], sig[:-1], mag[:-1], g4, dt, fexp, ferf)
        return np.concatenate([v, np.zeros((1, 9), dt)]), np.concatenate([s, np.zeros((1, 9))]), L
    o, d, alb, mu, sig, mag, g4 = (np.asarray(a, dt) for a in (o, d, alb, mu, sig, mag, g4))
    one = dt(1.0)
    c = mu - o
    bb = c - mu
    lo = (mu - (c - bb)) - (o + bb)                     # what the rounding of mu - o drops, exactly (two-sum), as the kernel keeps it
    # mubar = c . n as hi + lo, the kernel's compensated dot product (numpy has no fma: float64 stands for the exact products and sums).
    # A rounding error of mubar moves c_perp along n: second order in d2, but first order in a COMPONENT of c_perp that is small
    # against |c| |n_component| -- 2e-5 of such a component's addends in the grid scene with a plain float32 dot product.
    f64 = np.float64
    exact = (c.astype(f64) + lo.astype(f64)) @ d.astype(f64)
    mubar = exact.astype(dt)
    mlo = (exact - mubar.astype(f64)).astype(dt)
    cp = (c.astype(f64) - mubar.astype(f64)[:, None] * d.astype(f64)).astype(dt)       # one rounding: the kernel's fma
    cp = (cp.astype(f64) - mlo.astype(f64)[:, None] * d.astype(f64)).astype(dt) + lo
    d2 = (cp * cp).sum(1)
    inv_s = one / sig
    r = inv_s / dt(SQRT2)
    inv2s2 = one / (dt(2.0) * sig * sig)
    ex = fexp(-(d2 * inv2s2))
    Am = dt(K) * sig * ex
    A = Am * mag
    mr = mubar * r
    E = ferf(-mr)
    e1 = np.exp(-(mr * mr))
    if variant == "e1_sign":
        e1 = -e1
    G = alb[:, :3] @ g4[:3] if variant == "no_alpha" else alb @ g4
    kk = np.arange(-4, 1).astype(dt)
    q1 = inv_s if variant == "no_d2_term" else inv_s + d2 * inv_s * inv_s * inv_s
    mult = np.ones(n, dt)
    if variant == "double_absorber":
        mult[0] = 2
    val, S, L = np.zeros((n, 9), dt), np.zeros((n, 9)), np.zeros(4, dt)

    def add(rows, col, terms, axes):
        val[rows, col] += terms.sum(axes, dtype=dt)
        S[rows, col] += np.abs(terms).sum(axes, dtype=np.float64)

    eb = max(1, 400000 // (5 * max(n, 1)))
    for i0 in range(0, n, eb):
        sl = slice(i0, min(n, i0 + eb))
        s = mubar[sl, None] + kk[None, :] * sig[sl, None]
        x = (s[:, :, None] - mubar[None, None, :]) * r[None, None, :]
        D = E[None, None, :] - ferf(x)
        acc = (A[None, None, :] * D).sum(2, dtype=dt)
        t = sig[sl, None] * fexp(acc - (d2 * inv2s2)[sl, None] - (kk * kk / dt(2.0))[None, :])     # sigma_i (pdf / m_i) T_ik
        L += (alb[sl] * mag[sl, None]).T @ t.sum(1, dtype=dt)
        tm = t.copy()
        if variant == "no_k0":
            tm[:, 4] = 0
        if variant == "no_tail":
            tm[np.arange(sl.start, sl.stop) >= 4 * (n // 4)] = 0
        w = (G * mag)[sl, None] * tm
        # ---- to the emitter ----
        for ch in range(4):
            add(sl, ch, g4[ch] * mag[sl, None] * tm, 1)
        add(sl, 8, G[sl, None] * tm, 1)
        add(sl, 7, w * q1[sl, None], 1)
        for ax in range(3):
            add(sl, 4 + ax, -w * (cp[sl, ax] * inv_s[sl] * inv_s[sl])[:, None], 1)
        e2 = np.exp(-(x * x))
        ws = w[:, :, None] * (-(A * dt(CE) * r)[None, None, :] * e2)                                  # w_ik times the terms of S_ik
        if variant != "no_n_term":
            for ax in range(3):
                add(sl, 4 + ax, ws * d[ax], (1, 2))
        if variant != "no_k_term":
            add(sl, 7, ws * kk[None, :, None], (1, 2))
        # ---- to every absorber ----
        wa = w[:, :, None] * mult[None, None, :]
        if variant == "no_self_absorber":
            wa = wa * (np.arange(sl.start, sl.stop)[:, None, None] != np.arange(n)[None, None, :])
        rows = slice(0, n)
        add(rows, 8, wa * (Am[None, None, :] * D), (0, 1))
        AD = A[None, None, :] * D
        add(rows, 7, wa * (AD * q1[None, None, :] + (A * dt(CE) * inv_s)[None, None, :] * ((e1 * mr)[None, None, :] + e2 * x)), (0, 1))
        bn = (A * dt(CE) * r)[None, None, :] * (e2 - e1[None, None, :])
        for ax in range(3):
            add(rows, 4 + ax, wa * (-AD * (cp[:, ax] * inv_s * inv_s)[None, None, :] + bn * d[ax]), (0, 1))
    return val, S, L


# ---- the cull: which Gaussians a ray keeps, and which decisions float32 could make either way ----
def cull_x_of(g, cull_eps, exp_kind):
    sigma = g["sigma"].astype(np.float64)
    q = np.abs(sigma * g["magnitude"].astype(np.float64))
    cx = np.full(len(g), EXP_FLOOR[exp_kind])
    if cull_eps > 0:
        with np.errstate(divide="ignore"):
            cx = np.minimum(cx, np.log(q / (cull_eps * min(1.0, 4096.0 / max(len(g), 1)))))
    cx[q == 0] = -np.inf
    return cx


def undecided(o, d, g):
    """[N] bool: Gaussians within the float32 margin (ray_bundle_scenes.kept_range's band) of some ray's cull decision, under
    any cull_eps and Exp of the suite."""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    oc = g["mu"][:, :3].astype(np.float64)[None] - o[:, None]
    t = (oc * d[:, None]).sum(2)
    scale = 1.0 / (2.0 * g["sigma"].astype(np.float64) ** 2)[None]
    x = ((oc * oc).sum(2) - t * t) * scale
    band = 8.0 * 2.0 ** -24 * (oc * oc).sum(2) * scale + 1e-5 * np.abs(x)
    out = np.zeros(len(g), bool)
    for eps in EPS:
        for ek in (0, 1):
            out |= (np.abs(x - cull_x_of(g, eps, ek)[None]) <= band).any(0)
    return out


class GradScene:
    """g: the Gaussians; o, d: the bundle ([3] or [rays, 3] origins); gr: d(loss) / d(radiance) [rays, 4]; markers: Gaussians whose
    gradient the scene is about."""

    def __init__(self, name, g, o, d, gr, markers):
        self.name, self.g, self.o, self.d, self.gr, self.markers = name, g, np.asarray(o, np.float32), np.asarray(d, np.float32), gr, list(markers)

    def origin(self, r):
        return self.o if self.o.size == 3 else self.o[r]

    def lists(self, cull_eps=1e-9, exp_kind=1):
        keep = R.kept(self.o, self.d, self.g, cull_eps, exp_kind)
        return [np.nonzero(k)[0] for k in keep]


def settled(g, o, d, max_frac=0.05):
    """g without the Gaussians whose cull decision float32 could make either way for some ray; at most max_frac of g may go."""
    u = undecided(o, d, g)
    assert u.sum() <= max_frac * len(g), (int(u.sum()), len(g))
    return g[~u]


def seeded_gr(nrays, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(nrays, 4)).astype(np.float32)


ORIGIN = np.array([0.0, 0.0, -2.0], np.float32)


def small(oracle, n, seed=None):
    """n Gaussians of sigma 0.25-0.5 around the z axis in front of the origin, 5 rays through jittered centres.  From five on: one of
    magnitude 0 (index 1; no ray keeps it), one of negative magnitude (index 2), one BEHIND the origin (index 3; the cull goes by the
    distance to the line, so the rays keep it)."""
    rng = np.random.default_rng(7000 + n if seed is None else seed)
    for _ in range(20):
        mu = np.concatenate([rng.uniform(-0.4, 0.4, size=(n, 2)), rng.uniform(0.0, 1.5, size=(n, 1))], 1)
        sigma = rng.uniform(0.25, 0.5, n)
        mag = rng.uniform(0.5, 1.2, n)
        alb = rng.uniform(0.1, 1.0, size=(n, 4))
        if n >= 5:
            mag[1] = 0.0
            mag[2] = -0.6
            mu[3] = (0.1, -0.05, -3.0)
        g = oracle.gaussians(alb, mu, sigma, mag)
        target = mu[rng.integers(0, n, 5)] * [1, 1, 1] + rng.normal(size=(5, 3)) * 0.1
        target[:, 2] = np.abs(target[:, 2]) + 0.2
        d = normalise(target - ORIGIN.astype(np.float64))
        if not undecided(ORIGIN, d, g).any():
            sc = GradScene(f"small {n}", g, ORIGIN, d, seeded_gr(5, 100 + n), [])
            strength = np.abs(bundle_grad(sc, "libm-libm", 1e-9)[0]).max(1)
            sc.markers = list(np.argsort(-strength, kind="stable")[:min(n, 3)])      # the (up to) three Gaussians the loss leans on most
            return sc
    raise AssertionError("no draw without an undecided Gaussian")


STACK_O = np.array([0.0, 0.0, -1.0], np.float32)     # near: x = (s - mubar) r carries ulp(|c|) r of rounding, whatever the code


def stack_pair(oracle, k):
    """k Gaussians of sigma 0.2 in a row on the z axis (optical depth 1.5 in all) and, last in the list, a small one at (0.3, 0, 1).
    Ray 0 is aimed at the small one and keeps k + 1, ray 1 is aimed at (-0.3, 0, 1) and keeps the k of the row: RAY_PL (k = 32) and the
    long kernel's rounds of 64 and 128 emitters per lane set, one either side."""
    rng = np.random.default_rng(4100 + k)
    mu = np.stack([np.zeros(k), np.zeros(k), np.linspace(0.2, 1.4, k)], 1)
    sigma = np.full(k, 0.2)
    mag = rng.uniform(0.7, 1.3, k) * 1.5 / (k * K * 0.2)
    alb = rng.uniform(0.1, 1.0, size=(k + 1, 4))
    mu = np.concatenate([mu, [[0.3, 0.0, 1.0]]])
    sigma = np.concatenate([sigma, [0.04]])
    mag = np.concatenate([mag, [1.0]])
    g = oracle.gaussians(alb, mu, sigma, mag)
    d = normalise(np.array([[0.3, 0.0, 1.0], [-0.3, 0.0, 1.0]]) - STACK_O.astype(np.float64))
    assert not undecided(STACK_O, d, g).any()
    return GradScene(f"stack {k}|{k + 1}", g, STACK_O, d, seeded_gr(2, 200 + k), [k // 2, k - 1, k])


def wide(oracle, n=RAY_LCAP + 1):
    """ray_bundle_scenes.wide_stack: n wide, faint Gaussians that the axial ray keeps, all of them -- one more than the long kernel's LDS list."""
    sc = R.wide_stack(oracle, RAY_LCAP, n)
    o, d = R.wide_rays()
    d = d[:1]
    assert not undecided(o, d, sc.g).any()
    return GradScene(f"wide {n}", sc.g, o, d, seeded_gr(1, 300), sc.markers)


def grid_bundle(oracle, kind, nrays=130):
    """The 16 x 16 grid scene under ray_bundle_scenes' coherent bundle (one origin, rays through neighbouring Gaussians: lists shared by
    many lanes), from half a unit in front of the grid, or a scattered bundle (every lane its own rows), without the undecided Gaussians."""
    g0 = oracle.grid_scene(16)
    if kind == "coherent":
        o, d = R.coherent_rays(g0, nrays, origin=(0.0, 0.0, 0.5))
    else:                                           # per-ray origins on a sphere of radius 0.8 around the grid's centre, aimed at random Gaussians
        rng = np.random.default_rng(77)
        v = rng.normal(size=(nrays, 3))
        o = (np.array([0.0, 0.0, 1.0]) + 0.8 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        pick = rng.integers(0, len(g0), nrays)
        d = normalise(g0["mu"][pick, :3].astype(np.float64) + rng.normal(size=(nrays, 3)) * g0["sigma"][pick, None] - o.astype(np.float64))
    g = settled(g0, o, d)
    gr = seeded_gr(nrays, 400 + (kind == "coherent"))
    hits = R.kept(o, d, g).sum(0)
    return GradScene(f"grid16 {kind}", g, o, d, gr, list(np.argsort(-hits, kind="stable")[:4]))


@functools.lru_cache(maxsize=None)
def _suite(oracle):
    return ([small(oracle, n) for n in (1, 2, 3, 4, 5, 9)] + [stack_pair(oracle, k) for k in (RAY_PL, 64, 128)] + [wide(oracle)]
            + [grid_bundle(oracle, "coherent"), grid_bundle(oracle, "scattered")])


def suite(oracle):
    return _suite(oracle)


def scene(oracle, name):
    return next(s for s in suite(oracle) if s.name == name)


# ---- the model over a bundle ----
def _rows(g, idx):
    return g["albedo"][idx], g["mu"][idx, :3], g["sigma"][idx], g["magnitude"][idx]


def bundle_grad(sc, pair, cull_eps, rays=None, gr=None, variant=None, dt=np.float64, fexp=None, ferf=None):
    """The table [N, 9] and its S [N, 9] summed over the rays (all, or `rays`), and the radiance [rays, 4]."""
    ek, fk = PAIRS[pair]
    if fexp is None:
        fexp, ferf = np.exp, (erf_as if fk == 1 else erf)
    gr = sc.gr if gr is None else gr
    lists = sc.lists(cull_eps, ek)
    rays = range(len(sc.d)) if rays is None else rays
    val, S, L = np.zeros((len(sc.g), 9), dt), np.zeros((len(sc.g), 9)), np.zeros((len(sc.d), 4), dt)
    for r in rays:
        idx = lists[r]
        if len(idx):
            v, s, L[r] = ray_grad(sc.origin(r), sc.d[r], *_rows(sc.g, idx), gr[r], dt, fexp, ferf, variant)
            val[idx] += v
            S[idx] += s
    return val, S, L


_MODELS = {}


def model(sc, pair, cull_eps=1e-9):
    """(val, S) of the whole bundle in float64, computed once."""
    key = (sc.name, pair, cull_eps)
    if key not in _MODELS:
        _MODELS[key] = bundle_grad(sc, pair, cull_eps)[:2]
    return _MODELS[key]


S_FLOOR = 1e-20     # float32 flushes what falls below 1.2e-38: a component all of whose addends are that small (a Gaussian at the Exp floor with
                    # cull_eps = 0) may come out as 0 on the device.  Below S_FLOOR the ratio is not measured, and the bound is RHO * S_FLOOR.


def bound(S):
    return RHO * np.maximum(S, S_FLOOR)


def oracle_fns(oracle, pair):
    """The oracle's Exp / Erf of the pair, elementwise on float32 arrays."""
    ek, fk = PAIRS[pair]
    L = oracle.lib()

    def wrap(fn, kind):
        def f(x):
            x = np.asarray(x, np.float32)
            return np.array([fn(kind, v) for v in x.ravel().tolist()], np.float32).reshape(x.shape)
        return f
    return wrap(L.oracle_exp, ek), wrap(L.oracle_erf, fk)


def measured_ratio(oracle, sc, pair, cull_eps):
    """worst |g32 - g64| / S of the scene over its whole bundle."""
    rays = range(len(sc.d))
    fexp, ferf = oracle_fns(oracle, pair)
    v64, S, _ = bundle_grad(sc, pair, cull_eps, rays=rays)
    v32, _, _ = bundle_grad(sc, pair, cull_eps, rays=rays, dt=np.float32, fexp=fexp, ferf=ferf)
    on = S > S_FLOOR
    return float((np.abs(v32.astype(np.float64) - v64)[on] / S[on]).max()) if on.any() else 0.0


def forward64(sc, pair, cull_eps, g=None):
    """The radiance [rays, 4] of the model in float64, over the lists of the scene AS IT IS (held fixed) with the parameters of g."""
    g = sc.g if g is None else g
    ek, fk = PAIRS[pair]
    ferf = erf_as if fk == 1 else erf
    lists = sc.lists(cull_eps, ek)
    L = np.zeros((len(sc.d), 4))
    for r, idx in enumerate(lists):
        if len(idx):
            L[r] = ray_grad(sc.origin(r), sc.d[r], *g_rows64(g, idx), np.zeros(4), ferf=ferf)[2]
    return L


def g_rows64(g, idx):
    """Rows of a scene given as a structured array or as a dict of float64 arrays (finite differences move those)."""
    if isinstance(g, dict):
        return g["albedo"][idx], g["mu"][idx], g["sigma"][idx], g["magnitude"][idx]
    return _rows(g, idx)


def params64(g):
    return {"albedo": g["albedo"].astype(np.float64), "mu": g["mu"][:, :3].astype(np.float64), "sigma": g["sigma"].astype(np.float64),
            "magnitude": g["magnitude"].astype(np.float64)}


def table_of(grad):
    """Renderer.radiance_rays_grad's dict as the model's [N, 9] table."""
    return np.concatenate([np.asarray(grad["albedo"], np.float64), np.asarray(grad["mu"], np.float64),
                           np.asarray(grad["sigma"], np.float64)[:, None], np.asarray(grad["magnitude"], np.float64)[:, None]], 1)
