"""Model, cases and bound for the transmittance gradient bundles (vrt_hip_transmittance_bundle_grad*,
csrc/vrt_ray_trans_grad_kernel.hip): tests/test_gpu_trans_grad_bundles.py runs the cases on the GPU,
tests/test_trans_grad_bundle_scenes.py checks on the CPU that the model is the derivative it claims to be, that the bound is what this
file says, and that the cases can tell a wrong kernel from a right one.

The scenes, the kept lists (the cull rule in float64) and the `settled` filter are grad_bundle_scenes' (G).  For one ray (o, n) and the
list it keeps, held fixed, with c = mu - o, mubar = c.n, c_perp = c - mubar n, d2 = |c_perp|^2, r = 1 / (sqrt2 sigma), m = mubar r,
K = 1 / 0.79788456, C = 2 / sqrt(pi) (include/vrt_hip.h has the contract, DESIGN.md section 4 the derivation):
    A_j = K sigma_j mag_j exp(-d2_j / (2 sigma_j^2)),   x_kj = (s_k - mubar_j) r_j,   D_kj = Erf(-m_j) - Erf(x_kj)
    E_k = sum_j A_j D_kj,   T_k = Exp(E_k),   S_k = dE_k / ds_k = -sum_j A_j C r_j e2_kj,    e1_j = exp(-m_j^2), e2_kj = exp(-x_kj^2)
and with a weight w_k per sample (TGRAD_T: w_k = g_k T_k; TGRAD_DEPTH: w_k = -g_k / S_k, the implicit function theorem on T(depth) = tau)
    d mag_j = sum_k w_k (A_j / mag_j) D_kj
    d mu_j = sum_k w_k [-A_j D_kj c_perp_j / sigma_j^2 + A_j C r_j e2_kj n - A_j C r_j e1_j n]
    d sigma_j = sum_k w_k [A_j D_kj (1 / sigma_j + d2_j / sigma_j^3) + A_j C e1_j m_j / sigma_j + A_j C e2_kj x_kj / sigma_j]
and per sample d s_k = w_k S_k (TGRAD_T) or d tau_k = g_k / (T_k S_k) (TGRAD_DEPTH).  `ray_tgrad` is that list, addend by addend -- every
bracketed term above is an addend of its own, as the kernels sum the e1 W terms apart from Q and R, and a term in D counts as one in
Erf(-m_j) and one in Erf(x_kj), which float32 rounds one by one: per output component the value and S, the sum of the absolute values of
its addends.  The bound of a component is B = RHO_T * S.  In depth mode every addend carries its
sample's 1 / |S_k| through w_k; the levels are chosen where the slope T |S| is at least depth_bundle_scenes.SLOPE_MIN (`depth_levels`), so
that factor stays bounded.

RHO_T.  `ray_tgrad` runs in float32 as well, with the oracle's Exp / Erf of the pair for the forward quantities: the worst |g32 - g64| / S
over every case of this file (every ray, sample set and mode, both pairs, both cull_eps) is the float32 rounding of the formulas
themselves; RHO_T is 4 times that.  test_trans_grad_bundle_scenes.py::test_rho holds the measurement against the constant.
"""
import functools

import numpy as np

import depth_bundle_scenes as DB
import grad_bundle_scenes as G
from grad_bundle_scenes import CE, EPS, K, PAIRS, RAY_LCAP, RAY_PL, S_FLOOR, SQRT2  # noqa: F401
from transmittance_bundle_scenes import WIDE_S

TGRAD_T, TGRAD_DEPTH = 0, 1
SG = 4          # RAY_SG of csrc/vrt_ray_trans.hpp: samples per walk of a list
NSC = 512       # csrc/vrt_ray_trans_grad_kernel.hip: samples per chunk of the one-wave-per-ray kernel
# measured on the CPU (test_rho prints it): worst |g32 - g64| / S = 1.89e-5 (vcl, A&S) and 1.90e-5 (libm, libm), both on "T grid16
# scattered" (the coherent grid bundle: 1.5e-5): the grid's sigma is 1 / 32, x = (s - mubar) r carries ulp(mubar) r = 1.4e-6 of float32
# rounding, and e2 = exp(-x^2) of a sample four sigma and more from a Gaussian passes it on as 2 |x| dx.  Every other T-mode case is below
# 3.4e-6 and every depth-mode case below 2.8e-6 (a crossing lies inside the Gaussians that make it).  4 x 1.90e-5 = 7.6e-5: the
# measurement does NOT allow grad_bundle_scenes' RHO = 2.6e-5 (a radiance gradient samples a Gaussian within four sigma of its own
# centre), so the constant is this file's own.
RHO_T = 7.6e-5
NCOL = 5        # the table's columns 4..8: d mu xyz, d sigma, d magnitude
VARIANTS = ("no_e1W", "e1_sign", "no_d2_term", "no_R", "r_const", "c_not_perp", "depth_sign", "depth_TS", "no_last_sample", "no_last_entry")


def bound(S):
    return RHO_T * np.maximum(S, S_FLOOR)


def ray_tgrad(o, d, mu, sig, mag, s, g, wrt, dt=np.float64, fexp=np.exp, ferf=G.erf, variant=None):
    """One ray over one kept list (arrays of its n Gaussians in list order), ns samples s with d(loss) / d(T or depth) g.  Returns (val
    [n, 5], S [n, 5] float64, gs [ns], Sgs [ns] float64, T [ns], Sk [ns]).  dt, fexp, ferf: the number format and the Exp / Erf of the
    forward quantities; e1 and e2 are numpy's exp in dt.  variant: one of VARIANTS, a WRONG model."""
    n = len(sig)
    if variant == "no_last_entry" and n:
        v, S, gs, Sgs, T, Sk = ray_tgrad(o, d, mu[:-1], sig[:-1], mag[:-1], s, g, wrt, dt, fexp, ferf)
        return np.concatenate([v, np.zeros((1, NCOL), dt)]), np.concatenate([S, np.zeros((1, NCOL))]), gs, Sgs, T, Sk
    o, d, mu, sig, mag, s, g = (np.asarray(a, dt) for a in (o, d, mu, sig, mag, s, g))
    one = dt(1.0)
    # c, mubar and c_perp as the kernel's grad_gauss keeps them (grad_bundle_scenes.ray_grad says why)
    c = mu - o
    bb = c - mu
    lo = (mu - (c - bb)) - (o + bb)
    f64 = np.float64
    exact = (c.astype(f64) + lo.astype(f64)) @ d.astype(f64)
    mubar = exact.astype(dt)
    mlo = (exact - mubar.astype(f64)).astype(dt)
    cp = (c.astype(f64) - mubar.astype(f64)[:, None] * d.astype(f64)).astype(dt)
    cp = (cp.astype(f64) - mlo.astype(f64)[:, None] * d.astype(f64)).astype(dt) + lo
    d2 = (cp * cp).sum(1)
    if variant == "c_not_perp":
        cp = c
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
    q1 = inv_s if variant == "no_d2_term" else inv_s + d2 * inv_s * inv_s * inv_s
    # ---- the samples ----
    live = g != 0
    if wrt == TGRAD_DEPTH:
        live &= np.isfinite(s) & (s > 0)
    sv = np.where(live, s, dt(0.0))
    gv = np.where(live, g, dt(0.0))
    x = (sv[:, None] - mubar[None, :]) * r[None, :]       # the difference first: one rounding of a number of x's own size, not of m's
    D = E[None, :] - ferf(x)
    AD = A[None, :] * D
    T = fexp(AD.sum(1, dtype=dt))
    e2 = np.exp(-(x * x))
    Sadd = -(A * dt(CE) * r)[None, :] * e2
    Sk = Sadd.sum(1, dtype=dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        if wrt == TGRAD_DEPTH:
            ok = live & (Sk != 0)
            w = np.where(ok, (gv if variant == "depth_sign" else -gv) / (T * Sk if variant == "depth_TS" else Sk), dt(0.0))
            gs = np.where(ok, gv / (T * Sk), dt(0.0))
            Sgs = np.abs(gs).astype(f64)
        else:
            w = np.where(live, gv * T, dt(0.0))
            gs = w * Sk
            Sgs = np.abs(w[:, None] * Sadd).sum(1, dtype=f64)
    if variant == "no_last_sample" and len(w):
        w = w.copy()
        w[-1] = 0
    # ---- the addends, [ns, n] each ----
    val, S = np.zeros((n, NCOL), dt), np.zeros((n, NCOL))

    def add(col, terms, size=None):
        val[:, col] += terms.sum(0, dtype=dt)
        S[:, col] += np.abs(terms if size is None else size).sum(0, dtype=f64)

    # D is the difference of two Erf values, each rounded on its own: where both are saturated on the same side (a Gaussian far ahead of
    # or far behind a sample AND the origin) float32 gives D = 0 for a true 1e-12.  A term in D counts as two addends, in Erf(-m) and in Erf(x).
    Dsize = np.abs(E)[None, :] + np.abs(E[None, :] - D)
    wk = w[:, None]
    add(4, wk * (Am[None, :] * D), wk * (Am[None, :] * Dsize))
    add(3, wk * (AD * q1[None, :]), wk * (A[None, :] * Dsize * q1[None, :]))
    ACs = (A * dt(CE) * inv_s)[None, :]
    if variant not in ("no_e1W", "r_const"):
        add(3, wk * (ACs * (e1 * mr)[None, :]))
    if variant not in ("no_R", "r_const"):
        add(3, wk * (ACs * (e2 * x)))
    ACr = (A * dt(CE) * r)[None, :]
    for ax in range(3):
        add(ax, -wk * (AD * (cp[:, ax] * inv_s * inv_s)[None, :]), wk * (A[None, :] * Dsize * (cp[:, ax] * inv_s * inv_s)[None, :]))
        add(ax, wk * (ACr * e2) * d[ax])
        if variant != "no_e1W":
            add(ax, -wk * (ACr * e1[None, :]) * d[ax])
    return val, S, gs, Sgs, T, Sk


# ---- cases: a scene of grad_bundle_scenes, a mode, samples (or levels) and d(loss) / d(T or depth) ----
class Case:
    """sc: the GradScene; wrt; s: [ns] shared or [rays, ns] (T mode: sample distances; depth mode: None until depths are known);
    tau: depth mode's levels [rays, nt]; g: [rays, ns] float32."""

    def __init__(self, name, sc, wrt, s, g, tau=None):
        self.name, self.sc, self.wrt, self.s, self.g, self.tau = name, sc, wrt, s, g, tau

    @property
    def ns(self):
        return self.g.shape[1]

    def samples(self, r, s=None):
        s = self.s if s is None else s
        return s[r] if s.ndim == 2 else s


def seeded_g(nrays, ns, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(nrays, ns)).astype(np.float32)


def extent(sc, r, idx):
    """[lo, hi] along ray r of what it keeps: mubar -+ 2 sigma over its list (0, 1 for an empty list)"""
    if not len(idx):
        return 0.0, 1.0
    mubar = (sc.g["mu"][idx, :3].astype(np.float64) - sc.origin(r).astype(np.float64)) @ sc.d[r].astype(np.float64)
    sig = sc.g["sigma"][idx].astype(np.float64)
    return float((mubar - 2 * sig).min()), float((mubar + 2 * sig).max())


def sample_set(sc, ns, per_ray):
    """ns distances before, inside and behind what the rays keep: the recipe of transmittance_bundle_scenes' STACK_S and PROFILE_S (one
    sample at the origin, most inside, one behind everything) laid over each ray's own extent, since these scenes sit at other distances
    than the stacks those constants were made for.  ns = 1: inside.  [ns] from the bundle's extent, or [rays, ns] from each ray's."""
    if ns <= 2:
        frac = np.array([0.5]) if ns == 1 else np.array([0.35, 0.7])
    else:
        frac = np.concatenate([[np.nan], np.linspace(0.1, 0.9, ns - 2), [1.25]])      # NaN: the sample at the origin
    lists = sc.lists()
    ext = np.array([extent(sc, r, idx) for r, idx in enumerate(lists)])
    if not per_ray:
        ext = np.array([[ext[:, 0].min(), ext[:, 1].max()]])
    s = ext[:, :1] + frac[None, :] * (ext[:, 1:] - ext[:, :1])
    s[:, np.isnan(frac)] = 0.0
    s = np.maximum(s, 0.0).astype(np.float32)
    return np.ascontiguousarray(s if per_ray else s[0])


def positive(sc):
    """The scene with the magnitudes made positive (depth mode: T falls along every ray); the kept lists are the same"""
    g = sc.g.copy()
    g["magnitude"] = np.abs(g["magnitude"])
    return G.GradScene(sc.name + " +", g, sc.o, sc.d, sc.gr, sc.markers)


def _rows(g, idx):
    if isinstance(g, dict):
        return g["mu"][idx], g["sigma"][idx], g["magnitude"][idx]
    return g["mu"][idx, :3], g["sigma"][idx], g["magnitude"][idx]


def forward_T(sc, pair, r, idx, s, g=None):
    """T [ns] of ray r over the list idx in float64 with the parameters of g (the scene's, or a dict of float64 arrays)"""
    ferf = G.erf_as if PAIRS[pair][1] == 1 else G.erf
    s = np.atleast_1d(np.asarray(s, np.float64))
    return ray_tgrad(sc.origin(r), sc.d[r], *_rows(sc.g if g is None else g, idx), s, np.ones(len(s)), TGRAD_T, ferf=ferf)[4]


def root(sc, pair, r, idx, tau, g=None, tol=1e-13):
    """The depths [nt] at which ray r's float64 T falls to the levels tau (magnitudes >= 0), by bisection to tol; +inf where it never
    does, 0 where it starts there."""
    tau = np.atleast_1d(np.asarray(tau, np.float64))
    if not len(idx):
        return np.where(tau >= 1.0, 0.0, np.inf)
    mu, sig, _ = _rows(sc.g if g is None else g, idx)
    mubar = (np.asarray(mu, np.float64) - sc.origin(r).astype(np.float64)) @ sc.d[r].astype(np.float64)
    s_end = max(0.0, float((mubar + 6 * SQRT2 * np.asarray(sig, np.float64)).max()))
    T0, Tend = forward_T(sc, pair, r, idx, [0.0, s_end], g)
    lo, hi = np.zeros(len(tau)), np.full(len(tau), s_end)
    while (hi - lo).max() > tol:
        mid = 0.5 * (lo + hi)
        below = forward_T(sc, pair, r, idx, mid, g) <= tau
        hi, lo = np.where(below, mid, hi), np.where(below, lo, mid)
    return np.where(T0 <= tau, 0.0, np.where(Tend > tau, np.inf, hi))


def depth_levels(sc, nt, pair="libm-libm"):
    """[rays, nt] levels between 1 and each ray's T_inf, kept where the slope T |S| at the crossing is at least SLOPE_MIN (the condition of
    depth_bundle_scenes: the 1 / |S_k| of depth mode stays bounded) and replaced by 0 where it is not or the ray keeps nothing: a level no ray
    reaches, whose depth is +inf.  With nt >= 3 the last level of every ray is 1: its depth is 0.  Both must contribute exactly nothing."""
    out = np.zeros((len(sc.d), nt), np.float32)
    frac = np.linspace(0.15, 0.85, nt)
    for r, idx in enumerate(sc.lists()):
        if not len(idx):
            continue
        mu, sig, _ = _rows(sc.g, idx)
        mubar = (mu.astype(np.float64) - sc.origin(r).astype(np.float64)) @ sc.d[r].astype(np.float64)
        t_inf = forward_T(sc, pair, r, idx, [max(0.0, float((mubar + 6 * SQRT2 * sig).max()))])[0]
        t0 = forward_T(sc, pair, r, idx, [0.0])[0]
        tau = (t0 - frac * (t0 - t_inf)).astype(np.float32)
        s = root(sc, pair, r, idx, tau, tol=1e-9)
        fin = np.isfinite(s) & (s > 0)
        _, _, _, _, T, Sk = ray_tgrad(sc.origin(r), sc.d[r], *_rows(sc.g, idx), np.where(fin, s, 1.0), np.ones(nt), TGRAD_T)
        out[r] = np.where(fin & (T * np.abs(Sk) >= 2 * DB.SLOPE_MIN), tau, 0.0)     # twice the limit here: the A&S pair's crossing moves a little
        if nt >= 3:
            out[r, -1] = 1.0
    return out


def slope_ok(case, pair, depths):
    """[rays, ns] bool: a sample of a depth-mode case contributes nothing, or the slope T |S| there is at least SLOPE_MIN"""
    sc, out = case.sc, np.ones(case.g.shape, bool)
    for r, idx in enumerate(sc.lists()):
        s = depths[r].astype(np.float64)
        fin = np.isfinite(s) & (s > 0) & (case.g[r] != 0)
        if len(idx) and fin.any():
            T, Sk = ray_tgrad(sc.origin(r), sc.d[r], *_rows(sc.g, idx), np.where(fin, s, 1.0), np.ones(len(s)), TGRAD_T,
                              ferf=G.erf_as if PAIRS[pair][1] == 1 else G.erf)[4:6]
            out[r] = ~fin | (T * np.abs(Sk) >= DB.SLOPE_MIN)
    return out


SAMPLE_COUNTS = (1, 3, 4, 5, 9)          # the residues of RAY_SG, and two groups plus one
CHUNK_COUNTS = (NSC - 1, NSC, NSC + 1)   # the one-wave-per-ray kernel's chunking
CHUNK_SCENE = f"stack {RAY_PL}|{RAY_PL + 1}"


@functools.lru_cache(maxsize=None)
def _cases(oracle):
    out = []

    def both(name, sc, ns, per_ray, seed, s=None):
        g = seeded_g(len(sc.d), ns, seed)
        out.append(Case(f"T {name}", sc, TGRAD_T, sample_set(sc, ns, per_ray) if s is None else s, g))
        pos = positive(sc)
        out.append(Case(f"depth {name}", pos, TGRAD_DEPTH, None, g, tau=depth_levels(pos, ns)))

    for n in (1, 2, 3, 5, 9):
        both(f"small {n}", G.scene(oracle, f"small {n}"), 5, n % 2 == 1, 500 + n)
    for i, ns in enumerate(SAMPLE_COUNTS):
        both(f"small 9 ns={ns}", G.scene(oracle, "small 9"), ns, i % 2 == 0, 520 + ns)
    for k in (RAY_PL, 64):
        both(f"stack {k}|{k + 1}", G.scene(oracle, f"stack {k}|{k + 1}"), 5 if k == RAY_PL else 4, k == RAY_PL, 540 + k)
    both(f"wide {RAY_LCAP + 1}", G.scene(oracle, f"wide {RAY_LCAP + 1}"), len(WIDE_S), False, 560, s=WIDE_S)
    both("grid16 coherent", G.scene(oracle, "grid16 coherent"), 3, True, 570)
    both("grid16 scattered", G.scene(oracle, "grid16 scattered"), 5, True, 580)
    for ns in CHUNK_COUNTS:
        both(f"{CHUNK_SCENE} ns={ns}", G.scene(oracle, CHUNK_SCENE), ns, False, 600 + ns)
    return out


def cases(oracle):
    return _cases(oracle)


def case(oracle, name):
    return next(c for c in cases(oracle) if c.name == name)


PARITY = ([f"small {n}" for n in (1, 2, 3, 5, 9)] + [f"small 9 ns={ns}" for ns in SAMPLE_COUNTS] + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64)]
          + [f"wide {RAY_LCAP + 1}", "grid16 coherent", "grid16 scattered"] + [f"{CHUNK_SCENE} ns={ns}" for ns in CHUNK_COUNTS])


# ---- the model over a bundle ----
class Result:
    def __init__(self, nG, nrays, ns, dt=np.float64):
        self.val, self.S = np.zeros((nG, NCOL), dt), np.zeros((nG, NCOL))
        self.gs, self.Sgs, self.T = np.zeros((nrays, ns), dt), np.zeros((nrays, ns)), np.zeros((nrays, ns), dt)


def bundle_tgrad(case, pair, cull_eps, s=None, rays=None, g=None, variant=None, dt=np.float64, fexp=None, ferf=None, params=None):
    """The table [N, 5], its S, the per-sample output [rays, ns] and its S, and T, summed over the rays (all, or `rays`).  s: the samples
    (depth mode: the depths) when they are not the case's own; params: a dict of float64 arrays in place of the scene's rows."""
    ek, fk = PAIRS[pair]
    if fexp is None:
        fexp, ferf = np.exp, (G.erf_as if fk == 1 else G.erf)
    sc = case.sc
    g = case.g if g is None else g
    lists = sc.lists(cull_eps, ek)
    out = Result(len(sc.g), len(sc.d), g.shape[1], dt)
    for r in (range(len(sc.d)) if rays is None else rays):
        idx = lists[r]
        if len(idx):
            v, S, gs, Sgs, T, _ = ray_tgrad(sc.origin(r), sc.d[r], *_rows(sc.g if params is None else params, idx), case.samples(r, s), g[r], case.wrt,
                                            dt, fexp, ferf, variant)
            out.val[idx] += v
            out.S[idx] += S
            out.gs[r], out.Sgs[r], out.T[r] = gs, Sgs, T
        else:
            out.T[r] = 1
    return out


_DEPTHS = {}


def model_depths(case, pair, cull_eps=1e-9):
    """[rays, nt] float32: the crossings of the float64 model for a depth-mode case's levels (what the CPU tests stand in for the device's
    depths with), computed once."""
    key = (case.name, pair, cull_eps)
    if key not in _DEPTHS:
        sc = case.sc
        lists = sc.lists(cull_eps, PAIRS[pair][0])
        _DEPTHS[key] = np.stack([root(sc, pair, r, lists[r], case.tau[r], tol=1e-9) for r in range(len(sc.d))]).astype(np.float32)
    return _DEPTHS[key]


def samples_of(case, pair, cull_eps=1e-9):
    return case.s if case.wrt == TGRAD_T else model_depths(case, pair, cull_eps)


def measured_ratio(oracle, case, pair, cull_eps):
    """worst |g32 - g64| / S of the case over its whole bundle, table and per-sample output"""
    fexp, ferf = G.oracle_fns(oracle, pair)
    s = samples_of(case, pair, cull_eps)
    a = bundle_tgrad(case, pair, cull_eps, s=s)
    b = bundle_tgrad(case, pair, cull_eps, s=s, dt=np.float32, fexp=fexp, ferf=ferf)
    worst = 0.0
    for v64, v32, S in ((a.val, b.val, a.S), (a.gs, b.gs, a.Sgs)):
        on = S > S_FLOOR
        if on.any():
            worst = max(worst, float((np.abs(v32.astype(np.float64) - v64)[on] / S[on]).max()))
    return worst


def params64(g):
    return {"mu": g["mu"][:, :3].astype(np.float64), "sigma": g["sigma"].astype(np.float64), "magnitude": g["magnitude"].astype(np.float64)}


def table_of(grad):
    """Renderer.transmittance_bundle_grad's dict as the model's [N, 5] table"""
    return np.concatenate([np.asarray(grad["mu"], np.float64), np.asarray(grad["sigma"], np.float64)[:, None],
                           np.asarray(grad["magnitude"], np.float64)[:, None]], 1)
