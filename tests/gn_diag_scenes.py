"""Scenes, weights, the model and the bound for the Gauss-Newton diagonal bundles (vrt_hip_radiance_rays_gn_diag*,
csrc/vrt_ray_gn_diag_kernel.hip): tests/test_gpu_gn_diag.py runs them on the GPU, tests/test_gn_diag_scenes.py checks on the CPU that the
model is the diagonal of an explicit J^T W J, that the float32 restatement stays inside the bound, and that wrong models fall outside it.

The model.  For ray r and channel c, grad_bundle_scenes.ray_grad(..., g4 = e_c) is the Jacobian row v_c [n, 9] of L_c(r) over the ray's
kept list and S_c, the sum of the absolute values of its addends.  Then, in float64,
    D = sum_r sum_c w_rc v_c^2.
The bound per entry.  No number in it is new: RHO is grad_bundle_scenes.RHO (a row the device forms is within RHO S_c of v_c), the rest
is float32 arithmetic -- the square, the weight, and a sum of depth n_j (the rays that keep j) of non-negative addends:
    B = sum_r sum_c |w_rc| (2 |v_c| RHO S_c + (RHO S_c)^2) + (n_j + 8) 2^-24 sum_r sum_c |w_rc| v_c^2
with S floored as grad_bundle_scenes.bound floors it.  An ordered table sums a segment in depth ceil(n_j / 64) + 6 (include/vrt_hip.h),
which then stands for n_j.
"""
import functools

import numpy as np

import grad_bundle_scenes as G
from grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL, RHO, S_FLOOR  # noqa: F401

E4 = np.eye(4)
WRONG = ("channels_first", "rays_first", "no_weights", "no_alpha", "no_W", "no_zy")


# ---- scenes: the gradient suite, a pair of lists RAY_PL + 2 | RAY_PL + 1, and one list of exactly RAY_LCAP ----
@functools.lru_cache(maxsize=None)
def _suite(oracle):
    extra = [G.stack_pair(oracle, RAY_PL + 1), G.wide(oracle, RAY_LCAP)]
    return list(G.suite(oracle)) + extra


def suite(oracle):
    return _suite(oracle)


WORKSPACE_EXTRA = 76       # list positions beyond RAY_LCAP: more than one lane set of the last walk, and no multiple of it


@functools.lru_cache(maxsize=None)
def workspace_bundle(oracle):
    """ray_bundle_scenes.wide_stack of RAY_LCAP + WORKSPACE_EXTRA Gaussians under all three of wide_rays: three long rays at once, each
    with WORKSPACE_EXTRA list positions in its own workgroup's slot of the one-wave-per-ray kernel's workspace in device memory.  Not
    in NAMES: one case of its own in the GPU suite."""
    n = RAY_LCAP + WORKSPACE_EXTRA
    sc = G.R.wide_stack(oracle, RAY_LCAP, n)
    o, d = G.R.wide_rays()
    assert not G.undecided(o, d, sc.g).any()
    return G.GradScene(f"wide {n} x{len(d)}", sc.g, o, d, G.seeded_gr(len(d), 301), sc.markers)


def scene(oracle, name):
    return next(s for s in suite(oracle) if s.name == name)


NAMES = ([f"small {n}" for n in (1, 2, 3, 4, 5, 9)] + [f"stack {k}|{k + 1}" for k in (RAY_PL, RAY_PL + 1, 64, 128)]
         + [f"wide {RAY_LCAP}", f"wide {RAY_LCAP + 1}", "grid16 coherent", "grid16 scattered"])


def weights(sc, kind):
    """[rays, 4] float32 in [0.25, 4] from the scene's own seed ("seeded"), or None: the NULL weights, all 1"""
    if kind is None or kind == "null":
        return None
    seed = 9000 + sum(ord(ch) for ch in sc.name)
    return np.random.default_rng(seed).uniform(0.25, 4.0, size=(len(sc.d), 4)).astype(np.float32)


def w64(sc, w):
    return np.ones((len(sc.d), 4)) if w is None else np.asarray(w, np.float64).reshape(len(sc.d), 4)


# ---- the four rows of a ray ----
def ray_rows(o, d, alb, mu, sig, mag, dt=np.float64, fexp=np.exp, ferf=G.erf, variant=None):
    """(v [4, n, 9], S [4, n, 9]): the Jacobian rows of the four channels of one ray over one kept list, and their addend sums"""
    out = [G.ray_grad(o, d, alb, mu, sig, mag, E4[c], dt, fexp, ferf, variant)[:2] for c in range(4)]
    return np.stack([np.asarray(v, np.float64) for v, _ in out]), np.stack([s for _, s in out])


_ROWS = {}


def rows(sc, pair, cull_eps=1e-9, variant=None):
    """Per ray (idx, v [4, n, 9], S [4, n, 9]) in float64, computed once per (scene, pair, lists, variant)"""
    ek, fk = PAIRS[pair]
    lists = sc.lists(cull_eps, ek)
    key = (sc.name, pair, variant, tuple(l.tobytes() for l in lists))
    if key not in _ROWS:
        ferf = G.erf_as if fk == 1 else G.erf
        _ROWS[key] = [(idx,) + (ray_rows(sc.origin(r), sc.d[r], *G._rows(sc.g, idx), ferf=ferf, variant=variant) if len(idx)
                               else (np.zeros((4, 0, 9)), np.zeros((4, 0, 9)))) for r, idx in enumerate(lists)]
    return _ROWS[key]


def rows_without(sc, pair, cull_eps, what):
    """The rows with a group of terms left out, from ray_grad's own variants (the rows are linear in every group of addends):
    "no_W": the terms in W are those in e1, and e1_sign flips them: half the sum; "no_zy": the emitter's own z (no_n_term) and y
    (no_k_term): both variants drop one each."""
    base = rows(sc, pair, cull_eps)
    if what == "no_W":
        flip = rows(sc, pair, cull_eps, "e1_sign")
        return [(idx, 0.5 * (v + vf), s) for (idx, v, s), (_, vf, _) in zip(base, flip)]
    nn, nk = rows(sc, pair, cull_eps, "no_n_term"), rows(sc, pair, cull_eps, "no_k_term")
    return [(idx, vn + vk - v, s) for (idx, v, s), (_, vn, _), (_, vk, _) in zip(base, nn, nk)]


def depth_of(nj, ordered):
    nj = np.asarray(nj, np.float64)
    return np.where(nj > 0, np.ceil(nj / 64.0) + 6.0, 0.0) if ordered else nj


def diag_of(sc, per_ray, w, rays=None, ordered=False):
    """(D [N, 9], B [N, 9], n_j [N]) of the bundle (all rays, or `rays`) from its per-ray rows"""
    N = len(sc.g)
    w = w64(sc, w)
    D, lin, nj = np.zeros((N, 9)), np.zeros((N, 9)), np.zeros(N, np.int64)
    for r in (range(len(sc.d)) if rays is None else rays):
        idx, v, S = per_ray[r]
        if not len(idx):
            continue
        Sf = RHO * np.maximum(S, S_FLOOR)
        wr = w[r][:, None, None]
        D[idx] += (wr * v * v).sum(0)
        lin[idx] += (np.abs(wr) * (2.0 * np.abs(v) * Sf + Sf * Sf)).sum(0)
        nj[idx] += 1
    absD = D if (w >= 0).all() else None
    if absD is None:
        absD = np.zeros((N, 9))
        for r in (range(len(sc.d)) if rays is None else rays):
            idx, v, _ = per_ray[r]
            if len(idx):
                absD[idx] += (np.abs(w[r])[:, None, None] * v * v).sum(0)
    B = lin + (depth_of(nj, ordered)[:, None] + 8.0) * 2.0 ** -24 * absD
    return D, B, nj


_MODELS = {}


def model(sc, pair, cull_eps=1e-9, wkind="seeded", ordered=False):
    """(D, B, n_j) of the whole bundle, computed once"""
    key = (sc.name, pair, cull_eps, wkind, ordered)
    if key not in _MODELS:
        _MODELS[key] = diag_of(sc, rows(sc, pair, cull_eps), weights(sc, wkind), ordered=ordered)
    return _MODELS[key]


def summation_term(sc, pair, cull_eps=1e-9, wkind="seeded", ordered=False):
    """The part of B that belongs to the sum over the rays (and the square and the weight): what two summation orders of the same
    per-ray shares may differ by"""
    D, _, nj = model(sc, pair, cull_eps, wkind, ordered)
    return (depth_of(nj, ordered)[:, None] + 8.0) * 2.0 ** -24 * np.abs(D)


def wrong_model(sc, pair, cull_eps, w, which):
    """D of one of WRONG"""
    N = len(sc.g)
    w = w64(sc, w)
    per_ray = rows(sc, pair, cull_eps)
    if which in ("no_W", "no_zy"):
        return diag_of(sc, rows_without(sc, pair, cull_eps, which), w)[0]
    if which == "no_weights":
        return diag_of(sc, per_ray, None)[0]
    if which == "no_alpha":
        w3 = w.copy()
        w3[:, 3] = 0.0
        return diag_of(sc, per_ray, w3)[0]
    D = np.zeros((N, 9))
    if which == "channels_first":                       # (sum_c sqrt(w_c) v_c)^2 per ray
        for r, (idx, v, _) in enumerate(per_ray):
            if len(idx):
                D[idx] += (np.sqrt(w[r])[:, None, None] * v).sum(0) ** 2
        return D
    assert which == "rays_first"                        # the gradient table of channel c (g = sqrt(w_c) e_c), squared
    T = np.zeros((4, N, 9))
    for r, (idx, v, _) in enumerate(per_ray):
        if len(idx):
            T[:, idx] += np.sqrt(w[r])[:, None, None] * v
    return (T * T).sum(0)


# ---- the float32 restatement ----
def _memo(fn):
    """fn over float32 arrays, remembered per argument: the four channels of a ray evaluate Exp and Erf at the same points"""
    seen = {}

    def f(x):
        x = np.ascontiguousarray(x, np.float32)
        key = (x.shape, hash(x.tobytes()))
        if key not in seen:
            if len(seen) > 64:
                seen.clear()
            seen[key] = fn(x)
        return seen[key]
    return f


def restated32(oracle, sc, pair, cull_eps, w):
    """D with every row formed in float32 with the oracle's Exp / Erf of the pair (grad_bundle_scenes.measured_ratio's restatement of
    the kernel), squared, weighted and summed in float32 in ray order"""
    ek, _ = PAIRS[pair]
    fexp, ferf = (_memo(f) for f in G.oracle_fns(oracle, pair))
    w = w64(sc, w).astype(np.float32)
    D = np.zeros((len(sc.g), 9), np.float32)
    for r, idx in enumerate(sc.lists(cull_eps, ek)):
        if len(idx):
            for c in range(4):
                v = G.ray_grad(sc.origin(r), sc.d[r], *G._rows(sc.g, idx), E4[c], np.float32, fexp, ferf)[0].astype(np.float32)
                D[idx] += (w[r, c] * v) * v
    return D


def table9(table):
    """[N, 12] (or the dict grad_columns makes of it) as the model's [N, 9]"""
    if isinstance(table, dict):
        return G.table_of(table)
    return np.asarray(table, np.float64)[:, :9]
