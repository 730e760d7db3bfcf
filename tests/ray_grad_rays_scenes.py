"""The model of the ray rows of the gradient bundles (vrt_hip_radiance_rays_grad_rays*, vrt_hip_transmittance_bundle_grad_rays*):
d(loss) / d(origin) and the tangential d(loss) / d(direction) of every ray.  tests/test_gpu_ray_grad_rays.py runs the scenes on the GPU,
tests/test_ray_grad_rays_scenes.py checks on the CPU that the model is the derivative it claims to be, that the bound is what this file
says, and that the scenes tell a wrong kernel from a right one.

Scenes, cases and kept lists are grad_bundle_scenes' (G) and trans_grad_bundle_scenes' (T); the only geometry of this file's own is the
off-axis ray of `wide_off_axis`.  Every observable depends on a ray (o, n) through c_j = mu_j - o and n alone: with mubar_j = c_j . n,
c_perp_j = c_j - mubar_j n and ray r's share of row j's d mu written as v_j = a_j c_perp_j + b_j n,
    d(loss) / d(o) = -sum_j (a_j c_perp_j + b_j n)               (translation invariance)
    d(loss) / d(n) =  sum_j (b_j - a_j mubar_j) c_perp_j         (tangential: the derivative along normalise(n + eps t), t perpendicular to n)
over the ray's kept list, held fixed.  a_j and b_j are recovered from the per-ray rows of G.ray_grad / T.ray_tgrad: a_j = -mag_j M_j /
sigma_j^2 with M_j the row's d magnitude (how the kernels' grad_row forms it), and b_j = v_j . n since c_perp is perpendicular to n.

S, per component the sum of the absolute values of the addends, from the S of those rows (Smu, SM) in the same way: the addends of
d / d o are those of the d mu rows, S_o = sum_j Smu_j; b_j = v_j . n has the addends of v_j's three components weighed by |n|, Sb_j =
Smu_j . |n|, a_j has those of M_j, Sa_j = |mag_j| SM_j / sigma_j^2, and S_n = sum_j (Sb_j + Sa_j |mubar_j|) |c_perp_j|.  The bound of a
component is B = RHO_R * S.

RHO_R.  `ray_rows` runs in float32 as well (the rows of G.ray_grad / T.ray_tgrad in float32 with the oracle's Exp / Erf of the pair, then
the two sums above in float32): the worst |g32 - g64| / S over the suite -- every scene of G with every ray, every case of T in both
modes, both pairs, both cull_eps -- is the float32 rounding of the formulas themselves; RHO_R is 4 times that, for another summation
order, fma contraction, the wave's order of summation and the device's exp.  test_ray_grad_rays_scenes.py::test_rho_r holds the
measurement against the constant.
"""
import copy
import functools

import numpy as np

import grad_bundle_scenes as G
import trans_grad_bundle_scenes as T
from grad_bundle_scenes import EPS, PAIRS, RAY_LCAP, RAY_PL, S_FLOOR  # noqa: F401
from trans_grad_bundle_scenes import TGRAD_DEPTH, TGRAD_T  # noqa: F401

RAY_GRAD_STRIDE = 8
# measured on the CPU (test_rho_r prints it): worst |g32 - g64| / S = 1.447e-6 (vcl, A&S) and 1.457e-6 (libm, libm), both on "depth grid16
# coherent" (the radiance rows of the coherent grid bundle: 1.36e-6, "depth grid16 scattered": 1.1e-6, the radiance rows of the scattered
# grid bundle: 7.9e-7; the off-axis wide ray 6.3e-7 in depth mode; every other scene and case below 3.6e-7).  4 x 1.457e-6 = 5.9e-6.
# The ratio is smaller than RHO and RHO_T because S is larger: b = v . n counts the addends of all three components of v.
RHO_R = 5.9e-6
# wrong models: the first four are this file's own, the others are wrong variants of the rows underneath
VARIANTS = ("go_sign", "c_not_perp", "no_a_mubar", "no_W", "no_Z", "no_last_entry")
T_VARIANTS = ("go_sign", "c_not_perp", "no_a_mubar", "no_W", "no_last_entry", "no_last_sample", "depth_sign")


def bound(S):
    return RHO_R * np.maximum(S, S_FLOOR)


def geometry(o, d, mu, dt=np.float64):
    """(mubar [n], c_perp [n, 3], c [n, 3]) of a list against one ray, as the kernels' grad_gauss keeps them (G.ray_grad says why)"""
    o, d, mu = (np.asarray(a, dt) for a in (o, d, mu))
    f64 = np.float64
    c = mu - o
    bb = c - mu
    lo = (mu - (c - bb)) - (o + bb)
    exact = (c.astype(f64) + lo.astype(f64)) @ d.astype(f64)
    mubar = exact.astype(dt)
    mlo = (exact - mubar.astype(f64)).astype(dt)
    cp = (c.astype(f64) - mubar.astype(f64)[:, None] * d.astype(f64)).astype(dt)
    cp = (cp.astype(f64) - mlo.astype(f64)[:, None] * d.astype(f64)).astype(dt) + lo
    return mubar, cp, c


def rows_of(o, d, mu, sig, mag, v, Smu, M, SM, dt=np.float64, variant=None):
    """One ray's row [6] (d origin xyz, tangential d direction xyz) in dt and its S [6] float64, from the ray's d mu rows v [n, 3] (S: Smu)
    and d magnitude entries M [n] (S: SM) over its kept list.  variant: one of this file's own wrong models."""
    mubar, cp, c = geometry(o, d, mu, dt)
    n = np.asarray(d, dt)
    sig, mag, v, M = (np.asarray(a, dt) for a in (sig, mag, v, M))
    a = -(mag * M) / (sig * sig)
    b = (v * n[None, :]).sum(1, dtype=dt)
    go = -v.sum(0, dtype=dt)
    if variant == "go_sign":
        go = -go
    coef = b if variant == "no_a_mubar" else b - a * mubar
    gn = (coef[:, None] * (c if variant == "c_not_perp" else cp)).sum(0, dtype=dt)
    f64 = np.float64
    an = np.abs(n.astype(f64))
    Sb = (Smu * an[None, :]).sum(1)
    Sa = np.abs(mag.astype(f64)) * SM / (sig.astype(f64) ** 2)
    S_o = Smu.sum(0)
    S_n = ((Sb + Sa * np.abs(mubar.astype(f64)))[:, None] * np.abs(cp.astype(f64))).sum(0)
    return np.concatenate([go, gn]), np.concatenate([S_o, S_n])


def ray_rows(o, d, alb, mu, sig, mag, g4, dt=np.float64, fexp=np.exp, ferf=G.erf, variant=None):
    """The row of one ray of a radiance gradient bundle over one kept list: (row [6], S [6])."""
    own = variant in ("go_sign", "c_not_perp", "no_a_mubar")
    under = None if own or variant is None else {"no_W": None, "no_Z": "no_n_term", "no_last_entry": "no_last"}[variant]
    val, S, _ = G.ray_grad(o, d, alb, mu, sig, mag, g4, dt, fexp, ferf, under)
    v = val[:, 4:7]
    if variant == "no_W":       # the e1 W term of b changes sign with e1: the mean of both signs is the row without it
        v = (v + G.ray_grad(o, d, alb, mu, sig, mag, g4, dt, fexp, ferf, "e1_sign")[0][:, 4:7]) / dt(2.0)
    return rows_of(o, d, mu, sig, mag, v, S[:, 4:7], val[:, 8], S[:, 8], dt, variant if own else None)


def ray_trows(o, d, mu, sig, mag, s, g, wrt, dt=np.float64, fexp=np.exp, ferf=G.erf, variant=None):
    """The row of one ray of a transmittance gradient bundle (either mode) over one kept list: (row [6], S [6])."""
    own = variant in ("go_sign", "c_not_perp", "no_a_mubar")
    under = None if own or variant is None else {"no_W": "no_e1W"}.get(variant, variant)
    val, S = T.ray_tgrad(o, d, mu, sig, mag, s, g, wrt, dt, fexp, ferf, under)[:2]
    return rows_of(o, d, mu, sig, mag, val[:, 0:3], S[:, 0:3], val[:, 4], S[:, 4], dt, variant if own else None)


# ---- over a bundle ----
def bundle_rows(sc, pair, cull_eps=1e-9, rays=None, gr=None, variant=None, dt=np.float64, fexp=None, ferf=None):
    """(rows [nrays, 6], S [nrays, 6]) of a radiance gradient bundle; a ray that keeps nothing (or is not in `rays`): zeros."""
    ek, fk = PAIRS[pair]
    if fexp is None:
        fexp, ferf = np.exp, (G.erf_as if fk == 1 else G.erf)
    gr = sc.gr if gr is None else gr
    lists = sc.lists(cull_eps, ek)
    rows, S = np.zeros((len(sc.d), 6), dt), np.zeros((len(sc.d), 6))
    for r in (range(len(sc.d)) if rays is None else rays):
        idx = lists[r]
        if len(idx):
            rows[r], S[r] = ray_rows(sc.origin(r), sc.d[r], *G.g_rows64(sc.g, idx), gr[r], dt, fexp, ferf, variant)
    return rows, S


def bundle_trows(case, pair, cull_eps=1e-9, s=None, rays=None, g=None, variant=None, dt=np.float64, fexp=None, ferf=None):
    """(rows [nrays, 6], S [nrays, 6]) of a transmittance gradient bundle; s: the samples (depth mode: the depths) when not the case's own"""
    ek, fk = PAIRS[pair]
    if fexp is None:
        fexp, ferf = np.exp, (G.erf_as if fk == 1 else G.erf)
    sc = case.sc
    g = case.g if g is None else g
    lists = sc.lists(cull_eps, ek)
    rows, S = np.zeros((len(sc.d), 6), dt), np.zeros((len(sc.d), 6))
    for r in (range(len(sc.d)) if rays is None else rays):
        idx = lists[r]
        if len(idx):
            rows[r], S[r] = ray_trows(sc.origin(r), sc.d[r], *T._rows(sc.g, idx), case.samples(r, s), g[r], case.wrt, dt, fexp, ferf, variant)
    return rows, S


_MODELS = {}


def model(sc, pair, cull_eps=1e-9):
    key = ("R", sc.name, pair, cull_eps)
    if key not in _MODELS:
        _MODELS[key] = bundle_rows(sc, pair, cull_eps)
    return _MODELS[key]


def tmodel(case, pair, cull_eps=1e-9):
    """... of a case at the samples T.samples_of gives it (depth mode: the float64 model's crossings)"""
    key = ("T", case.name, pair, cull_eps)
    if key not in _MODELS:
        _MODELS[key] = bundle_trows(case, pair, cull_eps, s=T.samples_of(case, pair, cull_eps))
    return _MODELS[key]


def _ratio(v64, v32, S):
    on = S > S_FLOOR
    return float((np.abs(v32.astype(np.float64) - v64)[on] / S[on]).max()) if on.any() else 0.0


def measured_ratio(oracle, sc, pair, cull_eps):
    fexp, ferf = G.oracle_fns(oracle, pair)
    v64, S = bundle_rows(sc, pair, cull_eps)
    v32, _ = bundle_rows(sc, pair, cull_eps, dt=np.float32, fexp=fexp, ferf=ferf)
    return _ratio(v64, v32, S)


def measured_tratio(oracle, case, pair, cull_eps):
    fexp, ferf = G.oracle_fns(oracle, pair)
    s = T.samples_of(case, pair, cull_eps)
    v64, S = bundle_trows(case, pair, cull_eps, s=s)
    v32, _ = bundle_trows(case, pair, cull_eps, s=s, dt=np.float32, fexp=fexp, ferf=ferf)
    return _ratio(v64, v32, S)


def is_marker(rows, S):
    """[nrays] bool: the rays on which the bound of every component is at most 1e-3 of the row's largest component"""
    return bound(S).max(1) <= 1e-3 * np.abs(rows).max(1)


def from_device(rows):
    """The library's rows [nrays, RAY_GRAD_STRIDE] (or ray_grad_columns' dict) as the model's [nrays, 6]"""
    if isinstance(rows, dict):
        return np.concatenate([np.asarray(rows["origin"], np.float64), np.asarray(rows["dir"], np.float64)], 1)
    rows = np.asarray(rows, np.float64)
    return np.concatenate([rows[:, 0:3], rows[:, 4:7]], 1)


# ---- the scratch slot: an off-axis ray through the wide stack ----
@functools.lru_cache(maxsize=None)
def wide_off_axis(oracle):
    """G's `wide` scene (RAY_LCAP + 1 wide, faint Gaussians on the axis) under ONE ray that is not the axial one: on the axis the gradient
    nearly cancels by symmetry and the bound is 2-3 % of it.  The axial ray tilted by the smallest of a few angles at which the ray still
    keeps all RAY_LCAP + 1 with none undecided and is a marker ray (test_ray_grad_rays_scenes.py checks all three)."""
    base = G.scene(oracle, f"wide {RAY_LCAP + 1}")
    o = base.o
    axis = base.d[0].astype(np.float64)
    side = np.cross(axis, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    for tilt in (0.02, 0.05, 0.1, 0.2):
        d = G.normalise((axis + tilt * side)[None, :])
        if G.undecided(o, d, base.g).any():
            continue
        sc = G.GradScene(f"wide {RAY_LCAP + 1} off axis", base.g, o, d, base.gr, base.markers)
        if all(len(l) == RAY_LCAP + 1 for eps in EPS for ek in (0, 1) for l in sc.lists(eps, ek)) and is_marker(*bundle_rows(sc, "libm-libm")).all():
            return sc
    raise AssertionError("no tilt of the axial ray keeps the whole stack and meets the marker condition")


def wide_off_axis_case(oracle, mode):
    """T's wide case of the mode on the off-axis ray"""
    base = T.case(oracle, f"{mode} wide {RAY_LCAP + 1}")
    sc = wide_off_axis(oracle)
    if mode == "T":
        return T.Case(base.name + " off axis", sc, TGRAD_T, base.s, base.g)
    pos = T.positive(sc)
    return T.Case(base.name + " off axis", pos, TGRAD_DEPTH, None, base.g, tau=T.depth_levels(pos, base.ns))


def suite(oracle):
    """The radiance scenes: G's, the axial wide ray replaced by the off-axis one"""
    return [sc for sc in G.suite(oracle) if not sc.name.startswith("wide")] + [wide_off_axis(oracle)]


def scene(oracle, name):
    return next(s for s in suite(oracle) if s.name == name)


# ---- forward sums along moved rays (the derivative check), kept lists held fixed ----
def moved(sc, o, d):
    """sc with float64 rays o, d in place of its own; .lists() must not be asked of it (the lists are held fixed: pass them)"""
    out = copy.copy(sc)
    out.o, out.d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    return out


def unit64(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def tangents(n):
    """two unit vectors perpendicular to n and to each other"""
    n = np.asarray(n, np.float64)
    t1 = np.cross(n, np.eye(3)[np.argmin(np.abs(n))])
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(n, t1)


def radiance_loss(sc, pair, lists, r, o, n):
    """g . L of ray r of sc moved to (o, n), over lists[r]"""
    ferf = G.erf_as if PAIRS[pair][1] == 1 else G.erf
    L = G.ray_grad(o, n, *G.g_rows64(G.params64(sc.g), lists[r]), np.zeros(4), ferf=ferf)[2]
    return float((L * sc.gr[r].astype(np.float64)).sum())


# ---- the pose fit: a pinhole camera recovered from a target bundle by plain gradient steps on its six parameters ----
def rotation(w):
    """Rodrigues: the rotation by |w| about w"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)


class PoseFit:
    """`small 9` seen by a pinhole camera of 8 x 8 rays at G.ORIGIN looking along +z.  The pose is (t, w): origin G.ORIGIN + t, directions
    rotation(w) applied to the camera's own.  The target is the model's radiance at the true pose (t, w) = 0; the fit starts 0.05 units
    and 1 degree off and takes STEPS plain gradient steps of size H_T on t and H_W on w (chosen here, on the float64 model)."""
    STEPS = 20
    H_T, H_W = 0.002, 0.0005      # twice and more of either and the model's loss rises; with these it falls by 100 in 20 steps
    T0 = np.array([0.03, -0.03, 0.0264575])      # |T0| = 0.05
    W0 = np.array([0.0, np.deg2rad(1.0), 0.0])
    PAIR, EPS = "vcl-as", 1e-9

    def __init__(self, oracle):
        self.sc = G.scene(oracle, "small 9")
        u = np.linspace(-0.25, 0.25, 8)
        x, y = np.meshgrid(u, u)
        self.d0 = unit64(np.stack([x.ravel(), y.ravel(), np.ones(64)], 1))
        self.o0 = G.ORIGIN.astype(np.float64)
        self.target = self.radiance(np.zeros(3), np.zeros(3))[0]

    def rays(self, t, w):
        return self.o0 + t, self.d0 @ rotation(w).T

    def bundle(self, t, w):
        """the GradScene of the pose, rays in float32 as the library takes them"""
        o, d = self.rays(t, w)
        return G.GradScene("pose", self.sc.g, o.astype(np.float32), G.normalise(d), None, [])

    def radiance(self, t, w):
        """(L [64, 4] float64, the bundle)"""
        b = self.bundle(t, w)
        return G.forward64(b, self.PAIR, self.EPS), b

    def loss_and_grad(self, t, w):
        """the float64 model's loss sum (L - L*)^2 and its gradient in (t, w): d / dt = sum_r g_o, d / dw = sum_r d_r x g_n"""
        L, b = self.radiance(t, w)
        resid = L - self.target
        rows, _ = bundle_rows(b, self.PAIR, self.EPS, gr=2 * resid)
        d = b.d.astype(np.float64)
        return float((resid ** 2).sum()), rows[:, :3].sum(0), np.cross(d, rows[:, 3:]).sum(0)

    def run(self):
        """[STEPS + 1] losses of the float64 model along the fit"""
        t, w, out = self.T0.copy(), self.W0.copy(), []
        for _ in range(self.STEPS):
            l, gt, gw = self.loss_and_grad(t, w)
            out.append(l)
            t, w = t - self.H_T * gt, w - self.H_W * gw
        out.append(self.loss_and_grad(t, w)[0])
        return np.array(out)
