"""Scenes for the one-wave block kernel (csrc/vrt_block_kernel.hip: render_body) and a float64 model of the decisions it takes per
ray: which of its block's survivors a ray keeps (the lane cull) and which of those the budgeted prune (prune_list) drops again.
tests/test_gpu_block.py renders them on the GPU, tests/test_block_scenes.py checks on the CPU that they can see what they are meant
to see.  numpy and the oracle only: no GPU, no product import.

What the code does, level by level (vrt_kernels.hip, vrt_block_kernel.hip, vrt_kernels_common.hpp); thresholds are in x =
(|oc|^2 - mubar^2) / (2 sigma^2), cull_x = min(floor, ln(|sigma mag| / eps_eff)), eps_eff = cull_eps min(1, 4096 / N):
  tile   the reference's tile test AND cone_keeps(tile cone, cull_x)                    -- no slack: the whole scene enters
  cell   cone_keeps(cell cone, cull_x - ln(ref_n / total)),   total  = the tile's list
  block  cone_keeps(block cone, cull_x - ln(ref_n / n_list)), n_list = the cell's list
  lane   keep iff !(x > cull_x - ln(ref_n / cnt)),            cnt    = the BLOCK's survivors (not n_list)
  prune  (budget > 0 and the block's longest list <= 16) e_k = exp(cull_x_k - x_k); entry k goes iff the sum of all e_l <= e_k,
         itself included, is <= budget = kappa (ref_n or 4096/3) max(1, N / 4096) / max(1, largest finite |albedo|)
A threshold at the Exp floor (cull_x not below exp_floor_x) takes no slack, and such an entry is never pruned (its s_t is INFINITY).
cone_keeps is conservative (0.999 xmin - 1e-3 > threshold, xmin from a lower bound of the distance) and every level above the lane
has the smaller slack, so no level above drops what a lane would keep: the model restates them to COUNT (tile_entries, list_entries,
and cnt, which the lane threshold needs) and to report if one ever did.

What the kernel sees of x and of e, and the intervals the model derives from it:
  x    a.w = |oc|^2 and mubar^2 are fp32 numbers of size |oc|^2 (25 .. 40 here) formed by three products and two sums each; the ray
       direction carries three roundings of its own (difference, norm, divide) that enter mubar^2 twice.  At most 16 roundings of
       relative size 2^-24 of |oc|^2 reach the difference:  |dx| <= 16 2^-24 |oc|^2 / (2 sigma^2) + 2^-22 x   (the product with
       1/(2 sigma^2), itself rounded).  For sigma >= 2 that is below 4e-6, for the narrow Gaussians (sigma 0.04) up to 8e-3.
  cull_x  logf of an fp32 quotient: |dc| <= 2^-22 max(1, |cull_x|).  The slack is __logf of an fp32 quotient: 2e-5 covers the
       native logarithm's 1 ulp of log2 at arguments up to 1365.
  lane cull   sure iff |x - (cull_x - slack)| > dx + dc + 2e-5, else ambiguous.
  ln e   t = cull_x - x (|dt| <= dx + dc), biased up to t + 0.001 |t| + 1e-4 (three fp32 operations: 3 2^-24 |t|), rounded to fp16 --
       round to nearest, relative 2^-11: t >= 0 for a kept entry, so the biased value is at least 1e-4, a normal fp16 -- and passed
       through __expf, exp2 of an fp32 product: relative (|t| + 2) 2^-23 in e.  With d = dx + dc and r = (|t| + 2) 2^-22:
           ln e_lo = (1.001 (t - d) + 1e-4) (1 - 2^-11) - r        ln e_hi = (1.001 (t + d) + 1e-4) (1 + 2^-11) + r
       The relative width of [e_lo, e_hi] is width(t) = exp(ln e_hi - ln e_lo) - 1 ~ t 2^-10: 0.9 % at the default budget (t = ln
       8192 = 9.0), dominated by the fp16 rounding.  The kernel's sums of at most 16 such terms add 16 2^-24.
  prune  entry k is surely dropped iff the sum of e_hi over every entry that may be in the list and may be <= e_k fits the budget,
       surely kept iff the sum of e_lo over every entry that surely is in the list and surely <= e_k (itself included) does not.
       Bit-identical Gaussians (same centre, sigma and |sigma mag|) give bit-identical e on every ray: the model knows them as tied.
Every margin of the scenes (edge_margin, LANE_M) comes from these; none is tuned on the GPU.
"""
import numpy as np

from boundary_scenes import MARKER_FACTOR, PL, PRUNE_PL, TOL_NOCULL, Scene, _camera  # noqa: F401 (re-exported)

REF_N = float(np.float32(4096.0) / np.float32(3.0))     # Tuning::cull_ref_n
FLOOR_VCL = float(np.float32(87.3))                     # exp_floor_x(VRT_EXP_VCL)
PCAP = 96
EPS_TEST, EPS_DEFAULT = 1e-7, 1e-9
KAPPA = 6.0
U24, U11 = 2.0 ** -24, 2.0 ** -11
ERR_D2, ERR_SLACK, ERR_SUM = 16 * U24, 2e-5, 16 * U24
ERR_RSQ = 2.0 ** -21      # cosine and sine of a cone built from cone_ray's directions (tests/list_scenes.py)
KEPT, GONE, AMB, ABSENT = 1, 2, 3, 0
SQRT_2PI = 2.5066282746310002
WIDE_SIGMA = 200.0        # the faint Gaussians: x <= 6e-4 over the whole image, e constant to 0.06 %
LANE_M = 0.01             # family 6: either side of the lane threshold -- far above the 6e-4 of the image and the 3e-5 of the comparison


def budget(kappa, n, albedo_scale=1.0, ref_n=REF_N, eps=EPS_TEST):
    """CellGrid::prune_budget, in the host's fp32 operations (vrt_hip_frame.cpp, cell_grid)."""
    f = np.float32
    if not eps > 0.0:
        return 0.0
    return float(f(kappa) * (f(ref_n) if ref_n > 0 else f(4096.0) / f(3.0)) * max(f(1.0), f(n) / f(4096.0)) / f(albedo_scale))


def albedo_scale(g):
    a = np.abs(g["albedo"].astype(np.float32)).ravel()
    a = a[np.isfinite(a)]
    return float(max(1.0, a.max())) if a.size else 1.0


def ln_e_interval(t, d=0.0):
    """[ln e_lo, ln e_hi] of what prune_list sees for an entry with t = cull_x - x known to +-d (the module's derivation)."""
    t = np.asarray(t, np.float64)
    r = (np.abs(t) + 2.0) * 2.0 ** -22 + 3 * U24 * np.abs(t)
    lo = (t - d + 0.001 * np.abs(t - d) + 1e-4) * (1.0 - U11) - r
    hi = (t + d + 0.001 * np.abs(t + d) + 1e-4) * (1.0 + U11) + r
    return lo, hi


def width(t, d=4e-6):
    """Relative width of the interval [e_lo, e_hi] at t."""
    lo, hi = ln_e_interval(t, d)
    return float(np.exp(hi - lo) - 1.0)


def edge_margin(b):
    """m of the budget-edge scenes: three times the interval's relative width at t = ln(budget), the largest an entry there has."""
    return 3.0 * width(np.log(b))


# ---- what the kernel sees, in float64 ----
def geometry(sc, eps, floor=FLOOR_VCL, rays=True, scale_n=True):
    """floor: exp_floor_x of the frame's Exp kind.  rays=False leaves out the per-ray tables x and err_x (npix x n numbers: the list
    suite's images are large and its model asks for a ray's x cell by cell).  scale_n=False is the list suite's wrong variant of
    eps_eff, without the 4096 / N."""
    key = ("_geom", eps) if (floor, rays, scale_n) == (FLOOR_VCL, True, True) else ("_geom", eps, floor, rays, scale_n)
    if key in sc:
        return sc[key]
    f = np.float32
    g = sc.g
    o32 = sc.origin.astype(f)
    d = np.stack([np.asarray(a, np.float64) for a in sc.plane], 1) - o32.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    oc = (g["mu"][:, :3].astype(f) - o32).astype(np.float64)
    w2 = (oc * oc).sum(1)
    s32, m32 = g["sigma"].astype(f), g["magnitude"].astype(f)
    inv2s2 = (f(1.0) / (f(2.0) * s32 * s32)).astype(np.float64)
    q = (s32 * m32).astype(f)
    n = len(g)
    eps_eff = f(eps) * (min(f(1.0), f(4096.0) / f(max(n, 1))) if scale_n else f(1.0))
    cull_x = np.full(n, float(floor))
    with np.errstate(divide="ignore"):
        raw = np.log((np.abs(q) / eps_eff).astype(f).astype(np.float64)) if eps > 0.0 else np.full(n, np.inf)
    err_cull = 2.0 ** -22 * np.maximum(1.0, np.abs(np.where(np.isfinite(raw), raw, 0.0)))
    assert not (np.abs(raw - floor) <= err_cull).any()      # at the floor or below it: no scene leaves that to the logarithm's last bit
    cull_x = np.minimum(cull_x, raw)
    cull_x[q == 0] = -np.inf
    at_floor = ~(cull_x < floor)
    x = err_x = None
    if rays:
        mubar = d @ oc.T
        x = np.maximum(w2[None, :] - mubar * mubar, 0.0) * inv2s2[None, :]
        err_x = (ERR_D2 * w2 * inv2s2)[None, :] + 2.0 ** -22 * x
    # tied entries: bit-identical centre, sigma and |sigma mag|
    rows = np.concatenate([g["mu"][:, :3].astype(f).view(np.uint32), s32.view(np.uint32)[:, None], np.abs(q).view(np.uint32)[:, None]], 1)
    _, group = np.unique(rows, axis=0, return_inverse=True)
    sc[key] = Scene(d=d, oc=oc, w2=w2, inv2s2=inv2s2, q=q, cull_x=cull_x, err_cull=err_cull, floor=at_floor, x=x, err_x=err_x,
                    group=np.asarray(group).reshape(-1), eps_eff=float(eps_eff))
    return sc[key]


def _slack(ref_n, n):
    return float(np.log(ref_n / max(n, 1))) if ref_n > 0 else 0.0


def _threshold(G, slack):
    return np.where(G.floor, G.cull_x, G.cull_x - slack)


def _cone(rays, axis, extra=0.0):
    """make_cone (+ rect_cone's 1e-4) from the rays that span it."""
    co = rays @ axis
    si = np.linalg.norm(np.cross(rays, axis), axis=1)
    return axis, min(co.min(), 1.0) * 0.9999, si.max() * 1.001 + 1e-6 + extra


def _rect_cone(sc, G, x0, y0, x1, y1):
    at = lambda x, y: G.d[min(x + sc.w * y, sc.w * sc.h - 1)]
    corners = np.stack([at(x0, y0), at(x1, y0), at(x0, y1), at(x1, y1)])
    return _cone(corners, at((x0 + x1 + 1) // 2, (y0 + y1 + 1) // 2), 1e-4)


def _cone_keeps(G, cone, thr, idx, rsq=False):
    """cone_keeps for the candidates idx: (keep, sure).  rsq: the cone comes from cone_ray's directions (the list kernels' tile and
    cell cones), whose cosine and sine are off by up to ERR_RSQ each -- tests/list_scenes.py derives the term."""
    axis, cos_t, sin_t = cone
    tc = G.oc[idx] @ axis
    dperp = np.sqrt(np.maximum(0.0, G.w2[idx] - tc * tc))
    dmin = np.maximum(0.0, dperp * cos_t - np.abs(tc) * sin_t)
    v = dmin * dmin * G.inv2s2[idx] * 0.999 - 1e-3
    margin = np.where(dmin > 0.0, 2e-3 * (1.0 + np.abs(v)) + 8 * ERR_D2 * G.w2[idx] * G.inv2s2[idx], 0.0) + G.err_cull[idx] + ERR_SLACK
    if rsq:
        margin = margin + np.where(dmin > 0.0, 2.0 * dmin * G.inv2s2[idx] * ERR_RSQ * (dperp + np.abs(tc)), 0.0)
    return ~(v > thr[idx]), np.abs(v - thr[idx]) > margin


def _ref_tile_keeps(sc, G):
    """The reference's tile test (rt.cpp:29-69) for the one tile of tw = th = 2: centre 0, half extents 1."""
    V = np.asarray(sc.view, np.float64).reshape(4, 4)
    mu = np.concatenate([sc.g["mu"][:, :3].astype(np.float64), np.ones((len(sc.g), 1))], 1)
    v = mu @ V                                     # column-major storage: v_k = sum_i m[4 i + k] mu_i
    vz = v[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        sig = sc.g["sigma"].astype(np.float64) / vz
        keep = (vz >= 1.0) & (sig >= 1e-5) & (np.abs(v[:, 0] / vz) <= 1.0 + 3.3 * sig) & (np.abs(v[:, 1] / vz) <= 1.0 + 3.3 * sig)
        near = (np.abs(vz - 1.0) < 1e-4) | (np.abs(np.abs(v[:, 0] / vz) - 1.0 - 3.3 * sig) < 1e-4) | (np.abs(np.abs(v[:, 1] / vz) - 1.0 - 3.3 * sig) < 1e-4)
    return keep, ~near


def block_lanes(sc):
    """The 8x8 blocks of the image (one tile, cells of 32x32, blocks in the kernel's order): the 64 lanes' pixel indices."""
    assert sc.w % 8 == 0 and sc.h % 8 == 0 and sc.w <= 32 and sc.h <= 32
    lane = np.arange(64)
    return [(by * 8 + lane // 8) * sc.w + bx * 8 + lane % 8 for by in range(sc.h // 8) for bx in range(sc.w // 8)]


def plan(sc, eps=EPS_TEST, kappa=KAPPA, ref_n=REF_N):
    """The model's frame: per ray the status of every Gaussian (ABSENT | KEPT | GONE: in the lane's list and pruned | AMB), the
    statistics it implies, and what the levels above the lane did."""
    key = ("_plan", eps, kappa, ref_n)
    if key in sc:
        return sc[key]
    G, n, npix = geometry(sc, eps), len(sc.g), sc.w * sc.h
    unsure = 0
    keep, sure = _ref_tile_keeps(sc, G)
    unsure += int((~sure).sum())
    tile = np.flatnonzero(keep)
    k2, s2 = _cone_keeps(G, _rect_cone(sc, G, 0, 0, sc.w - 1, sc.h - 1), _threshold(G, 0.0), tile)
    unsure += int((~s2).sum())
    tile = tile[k2]
    k3, s3 = _cone_keeps(G, _rect_cone(sc, G, 0, 0, min(32, sc.w) - 1, min(32, sc.h) - 1), _threshold(G, _slack(ref_n, len(tile))), tile)
    unsure += int((~s3).sum())
    cell = tile[k3]
    B = budget(kappa, n, albedo_scale(sc.g), ref_n, eps)
    status = np.zeros((npix, n), np.uint8)
    blocks, above = [], 0
    tile_entries = list_entries = 0
    lane_lo = lane_hi = pairs_lo = pairs_hi = max_lo = max_hi = 0
    for lanes in block_lanes(sc):
        c = G.d[lanes[[27, 28, 35, 36]]].sum(0)
        k4, s4 = _cone_keeps(G, _cone(G.d[lanes], c / np.linalg.norm(c)), _threshold(G, _slack(ref_n, len(cell))), cell)
        unsure += int((~s4).sum())
        surv = cell[k4]
        cnt = len(surv)
        assert cnt <= PCAP
        tile_entries += len(cell)
        list_entries += cnt
        thr = _threshold(G, _slack(ref_n, cnt))
        # would a lane keep, at its own threshold, what a level above dropped?
        gone = np.setdiff1d(np.arange(n), surv)
        above += int((~(G.x[lanes][:, gone] > thr[gone][None, :] + G.err_x[lanes][:, gone])).any(0).sum()) if len(gone) else 0
        x, ex = G.x[lanes][:, surv], G.err_x[lanes][:, surv]
        lane_margin = ex + G.err_cull[surv][None, :] + ERR_SLACK
        in_sure = x <= thr[surv][None, :] - lane_margin
        in_may = x <= thr[surv][None, :] + lane_margin
        assert in_may.sum(1).max() <= PL, "a block of these scenes never goes to the dense path"
        st = np.where(in_sure, KEPT, np.where(in_may, AMB, ABSENT)).astype(np.uint8)
        nmax_lo, nmax_hi = int(in_sure.sum(1).max()), int(in_may.sum(1).max())
        if B > 0.0 and nmax_hi <= PRUNE_PL and cnt:
            floor = G.floor[surv]
            t = G.cull_x[surv][None, :] - x
            lo, hi = ln_e_interval(np.where(in_may & ~floor[None, :], t, 0.0), ex + G.err_cull[surv][None, :])
            e_lo, e_hi = np.exp(lo), np.exp(hi)
            tied = G.group[surv][:, None] == G.group[surv][None, :]
            may_le = tied[None] | (e_lo[:, :, None] <= e_hi[:, None, :])            # [ray, l, k]: e_l <= e_k possible
            sure_le = tied[None] | (e_hi[:, :, None] <= e_lo[:, None, :])
            cand = (in_may & ~floor[None, :])
            upper = (np.where(cand, e_hi, 0.0)[:, :, None] * may_le).sum(1) * (1.0 + ERR_SUM)
            lower = (np.where(in_sure & ~floor[None, :], e_lo, 0.0)[:, :, None] * sure_le).sum(1) * (1.0 - ERR_SUM)
            dropped, stays = cand & (upper <= B), in_sure & (floor[None, :] | (lower > B))
            st = np.where(dropped, GONE, np.where(stays, KEPT, np.where(in_may, AMB, ABSENT))).astype(np.uint8)
        elif B > 0.0 and nmax_lo <= PRUNE_PL < nmax_hi:
            st = np.where(in_may, AMB, ABSENT).astype(np.uint8)
        status[np.ix_(lanes, surv)] = st
        nl_lo, nl_hi = (st == KEPT).sum(1), ((st == KEPT) | (st == AMB)).sum(1)
        lane_lo, lane_hi = lane_lo + int(nl_lo.sum()), lane_hi + int(nl_hi.sum())
        pairs_lo, pairs_hi = pairs_lo + int((nl_lo * nl_lo).sum()), pairs_hi + int((nl_hi * nl_hi).sum())
        max_lo, max_hi = max_lo + int(nl_lo.max()), max_hi + int(nl_hi.max())
        blocks.append(Scene(lanes=lanes, survivors=surv, cnt=cnt, n_list=len(cell), nmax=(nmax_lo, nmax_hi), left=(int(nl_lo.max()), int(nl_hi.max()))))
    ambiguous = (status == AMB).any(1)
    sc[key] = Scene(status=status, ambiguous=ambiguous, n_ambiguous=int(ambiguous.sum()), budget=B, blocks=blocks, n_blocks=len(blocks),
                    tile_entries=tile_entries, list_entries=list_entries, lane_entries=(lane_lo, lane_hi), lane_pairs=(pairs_lo, pairs_hi),
                    lane_max_entries=(max_lo, max_hi), above_drops=above, cone_unsure=unsure,
                    n_pruned=int((status == GONE).sum()), n_kept=int((status == KEPT).sum()))
    return sc[key]


def kept_sets(p):
    """{kept set in scene order: pixels} over the unambiguous rays."""
    out = {}
    for pix in np.flatnonzero(~p.ambiguous):
        out.setdefault(tuple(np.flatnonzero(p.status[pix] == KEPT)), []).append(pix)
    return {k: np.array(v, np.uint32) for k, v in out.items()}


def oracle_radiance(oracle, sc, p, threads=8):
    """The oracle's radiance of every ray over the model's kept set for that ray (float64, [npix, 4]; NaN on ambiguous rays) and
    the packed pixels."""
    rad = np.full((sc.w * sc.h, 4), np.nan)
    img = np.zeros(sc.w * sc.h, np.uint32)
    for kept, pix in kept_sets(p).items():
        if len(kept) == 0:
            rad[pix] = 0.0
            continue
        im, r = oracle.render(sc.w, sc.h, sc.plane, sc.origin, np.ascontiguousarray(sc.g[list(kept)]), None, pixels=pix, threads=threads)
        rad[pix] = r.astype(np.float64)
        img[pix] = im[pix]
    return rad, img


def checked_pixels(p, rad):
    """The unambiguous rays, brightest first: every block has some."""
    pix = np.flatnonzero(~p.ambiguous)
    assert all((~p.ambiguous[b.lanes]).any() for b in p.blocks)
    return pix[np.argsort(-rad[pix, :3].sum(1), kind="stable")].astype(np.uint32)


# ---- the scenes ----
def _finish(oracle, w, h, alb, mu, sigma, mag, **extra):
    plane, view, origin = _camera(oracle, w, h)
    g = oracle.gaussians(np.asarray(alb, np.float32), mu, sigma, mag)
    return Scene(g=g, n=len(g), w=w, h=h, tw=2.0, th=2.0, plane=plane, view=view, origin=origin, **extra)


def _brights(rng, n):
    """n wide Gaussians around (0, 0, 1) that every ray keeps and no budget reaches: sigma mag exp(-x) / eps >= 1.6e5 over the
    whole image at eps 1e-7 (x <= 1.8 in the corners), against a budget of 8.2e3 (8.2e4 at kappa 60)."""
    mu = rng.normal(size=(n, 3)) * 0.15 + np.array([0, 0, 1.0])
    sigma = rng.uniform(2.2, 2.8, n)
    mag = rng.uniform(0.10, 0.16, n) / sigma
    alb = rng.uniform(0.2, 1.0, size=(n, 4))
    return alb, mu, sigma, mag


def _faint(e, eps_eff, centre=(0.0, 0.0, 1.0), sigma=WIDE_SIGMA, alb=(1.0, 1.0, 1.0, 1.0)):
    """One wide faint Gaussian with sigma mag / eps_eff = e: (albedo, mu, sigma, mag)."""
    return alb, centre, sigma, e * eps_eff / sigma


def mixed(oracle, seed, n_bright, faints, pos="last", eps=EPS_TEST, w=16, h=16, scene_n=None, narrow=(), **extra):
    """n_bright wide bright Gaussians and the `faints` -- (e in units of eps_eff, or a full (albedo, mu, sigma, mag) row) -- as one
    run at the first, a middle or the last list position; `narrow`: rows appended behind both.  scene_n: the scene's length when it
    is padded elsewhere (eps_eff depends on it)."""
    rng = np.random.default_rng(seed)
    alb, mu, sigma, mag = (list(a) for a in _brights(rng, n_bright))
    n = scene_n or (n_bright + len(faints) + len(narrow))
    eps_eff = eps * min(1.0, 4096.0 / n)
    rows = [_faint(f, eps_eff) if np.isscalar(f) else f for f in faints]
    at = {"first": 0, "middle": n_bright // 2, "last": n_bright}[pos]
    for j, (a, m, s, q) in enumerate(list(rows)):
        alb.insert(at + j, a); mu.insert(at + j, m); sigma.insert(at + j, s); mag.insert(at + j, q)
    for a, m, s, q in narrow:
        alb.append(a); mu.append(m); sigma.append(s); mag.append(q)
    return _finish(oracle, w, h, np.array(alb), np.array(mu), np.array(sigma), np.array(mag), faint_at=list(range(at, at + len(rows))), eps=eps, **extra)


def on_ray(sc_or_cam, pix, depth=5.0):
    """The point at `depth` along the view axis on the ray of pixel pix."""
    plane, origin = sc_or_cam
    o = origin.astype(np.float64)
    d = np.array([plane[0][pix], plane[1][pix], plane[2][pix]], np.float64) - o
    return o + d * (depth / d[2])


EDGE_WEIGHTS = {1: (1.0,), 2: (1.0, 1.25), 3: (1.0, 1.25, 1.5), 5: (1.0, 1.25, 1.5, 1.75, 2.0)}


def budget_edge(oracle, k, side, pos, eps=EPS_TEST):
    """Family 1: k faint entries (weights 1 : 1.25 : ...) whose sum is budget (1 + side m), among five bright ones."""
    B = budget(KAPPA, 5 + k)
    wts = np.array(EDGE_WEIGHTS[k])
    es = wts / wts.sum() * B * (1.0 + side * edge_margin(B))
    sc = mixed(oracle, 100 + k, 5, list(es), pos, eps)
    sc.update(family=1, side=side, k=k, expect_dropped=k if side < 0 else k - 1)
    return sc


def instantiation(oracle, nmax, pos="last", eps=EPS_TEST):
    """Family 2: a list of nmax on every ray, one entry of it (e = 3000) prunable."""
    sc = mixed(oracle, 200 + nmax, nmax - 1, [3000.0], pos, eps)
    sc.update(family=2, nmax=nmax)
    return sc


def ragged(oracle, kind, eps=EPS_TEST):
    """Family 3.  'narrow': a narrow bright Gaussian (sigma 0.3) on the ray of pixel (5, 6): a dozen lanes of block 0 keep it, so nl
    differs per lane, and its fringe is prunable.  'cross': a faint Gaussian of sigma 3 whose e falls from 12000 at its centre
    through the budget (8192) 4 pixels out, inside all four blocks.  'both': the two together among seven bright ones."""
    cam = _camera(oracle, 16, 16)
    eps_eff = eps
    narrow = [((1.0, 0.4, 0.2, 1.0), on_ray((cam[0], cam[2]), 6 * 16 + 5), 0.3, 1.0 * eps / EPS_TEST)]
    cross = [_faint(12000.0, eps_eff, centre=(0.11, -0.07, 1.0), sigma=3.0)]
    n_bright = {"narrow": 9, "cross": 4, "both": 7}[kind]
    sc = mixed(oracle, 300 + n_bright, n_bright, cross if kind != "narrow" else [], "middle", eps, narrow=narrow if kind != "cross" else [])
    sc.update(family=3, kind=kind)
    return sc


def ties(oracle, copies, fit, eps=EPS_TEST):
    """Family 4: a smaller entry (2000) and `copies` bit-identical ones: all of it fits the budget of 8192 (fit: 7600, 7400) or the
    smaller one with one copy does (7000, 5000) and with all copies does not (12000, 11000)."""
    e = {(2, True): 2800.0, (3, True): 1800.0, (2, False): 5000.0, (3, False): 3000.0}[(copies, fit)]
    sc = mixed(oracle, 400 + copies, 4, [2000.0] + [e] * copies, "middle", eps)
    sc.update(family=4, copies=copies, fit=fit, tied=sc.faint_at[1:])
    return sc


def nothing_to_do(oracle, kind, eps=EPS_TEST):
    """Family 5.  'none': bright entries only -- the __ballot(least <= budget) == 0 exit.  'one-lane': four blocks, and a very
    narrow faint Gaussian (sigma 0.04, e = 3000 on its own ray, nothing 0.6 away) on the ray of pixel (4, 4): one lane of block 0."""
    cam = _camera(oracle, 16, 16)
    narrow = [] if kind == "none" else [((1.0, 1.0, 1.0, 1.0), on_ray((cam[0], cam[2]), 4 * 16 + 4), 0.04, 3000.0 * eps / 0.04)]
    sc = mixed(oracle, 500, 6, [], "last", eps, narrow=narrow)
    sc.update(family=5, kind=kind, lane_pixel=4 * 16 + 4)
    return sc


def lane_threshold(oracle, eps=EPS_TEST):
    """Family 6 (prune off): block 0 keeps 6 bright + 2 faint candidates (cnt 8), blocks 1 .. 3 one narrow Gaussian more each (cnt 9,
    the cell's list 11).  The faint ones carry e = (ref_n / 8) (1 +- LANE_M): block 0 keeps one and drops the other, the blocks with
    cnt 9 (threshold ref_n / 9) keep both -- and so would block 0 if it took the cell's 11 for cnt."""
    cam = _camera(oracle, 16, 16)
    narrow = [((0.3, 1.0, 0.4, 1.0), on_ray((cam[0], cam[2]), py * 16 + px), 0.1, 10.0 * eps / EPS_TEST) for px, py in ((12, 3), (3, 12), (12, 12))]
    sc = mixed(oracle, 600, 6, [REF_N / 8 * (1 + LANE_M), REF_N / 8 * (1 - LANE_M)], "middle", eps, narrow=narrow)
    sc.update(family=6)
    return sc


FACTOR_FAINTS = (600.0, 650.0, 2500.0, 3000.0, 20000.0, 40000.0)    # cumulative 1250, 3750, 6750, 26750, 66750
FACTOR_DROPS = {0.0: 0, 1.0: 2, 6.0: 4, 60.0: 6}                    # budgets 0, 1365, 8192, 81920


def factors(oracle, kind="plain", eps=EPS_TEST):
    """Family 7: six faint entries in steps, five bright ones.  'albedo4': one albedo component of 4 (the budget a quarter: 2048 --
    1250 fits, 3750 does not); 'albedo-inf': an infinite component on top, which is ignored; 'negative': the 2500 with a negative
    magnitude; 'large': the scene padded to 8192 with Gaussians far outside the view (eps_eff halves, e doubles: 1200, 1300, 5000,
    6000 sum to 13500, inside the doubled budget of 16384 and outside 8192)."""
    n_scene = 8192 if kind == "large" else None
    sc = mixed(oracle, 700, 5, [e * (2.0 if kind == "large" else 1.0) for e in FACTOR_FAINTS], "middle", eps, scene_n=n_scene)
    g = sc.g.copy()
    if kind in ("albedo4", "albedo-inf"):
        g["albedo"][0, 1] = 4.0
    if kind == "albedo-inf":
        g["albedo"][1, 2] = np.inf
    if kind == "negative":
        g["magnitude"][sc.faint_at[2]] *= -1.0
    if kind == "large":
        rng = np.random.default_rng(701)
        pad = np.zeros(8192 - len(g), g.dtype)
        side = rng.choice([-1.0, 1.0], len(pad))
        pad["mu"][:, 0], pad["mu"][:, 1], pad["mu"][:, 2] = side * rng.uniform(50.0, 100.0, len(pad)), rng.uniform(-20.0, 20.0, len(pad)), 1.0
        pad["sigma"], pad["magnitude"], pad["albedo"] = 0.1, 1.0, 0.5
        g = np.concatenate([g[:4], pad[:4000], g[4:], pad[4000:]])          # the visible ones keep their order, far apart in the scene
        sc["faint_at"] = list(np.flatnonzero(np.isclose(g["sigma"], WIDE_SIGMA)))
    sc.update(g=np.ascontiguousarray(g), n=len(g), family=7, kind=kind)
    return sc


def floor_entries(oracle):
    """Family 8, cull_eps = 1e-38 on 32x32 pixels: Gaussians far down the view axis, so that x grows from 0 at the image centre to
    beyond every threshold towards its edge.  sigma mag = 1: cull_x is clamped to the floor (87.3), no slack, never pruned -- kept on
    every ray with x <= 87.3, though e = exp(87.3 - x) is below the budget from x = 78.3 on.  sigma mag = 1e-3: cull_x = 80.6; the
    lane keeps x <= 80.6 - ln(ref_n / cnt), and the prune takes what has x >= 80.6 - ln(budget) = 71.6: a ring of rays."""
    alb = [(1.0, 1.0, 1.0, 1.0)] * 5
    mu = [(0.0, 0.0, 16.0), (0.02, -0.01, 21.0), (0.0, 0.0, 17.0), (-0.015, 0.01, 23.0), (0.0, 0.0, 1.0)]
    sigma = np.array([0.97, 1.046, 1.16, 1.33, 2.5])      # chosen with the model alone: no cone decision and no ray within its margin
    q = np.array([1.0, 1.0, 1e-3, 1e-3, 0.1])
    sc = _finish(oracle, 32, 32, alb, mu, sigma, q / sigma, faint_at=[2, 3], eps=1e-38)
    sc.update(family=8)
    return sc


def tie_stack(oracle, k, eps=EPS_TEST):
    """k bit-identical faint Gaussians (e = 3000) and nothing else: every entry of every list is tied with every other, so the
    kernel's `below` is the sum of k equal fp32 numbers, added one after the other."""
    sc = mixed(oracle, 900, 0, [3000.0] * k, "last", eps)
    sc.update(family=4, copies=k)
    return sc


def running_sum32(e, k):
    """e + e + ... (k terms) as prune_list adds them: fp32, left to right, from 0."""
    total = np.float32(0.0)
    for _ in range(k):
        total = np.float32(total + np.float32(e))
    return total


_scenes = {}
BUILDERS = {"edge": budget_edge, "inst": instantiation, "ragged": ragged, "ties": ties, "nothing": nothing_to_do, "lane": lane_threshold,
            "factors": factors, "floor": floor_entries, "stack": tie_stack}


def scene(oracle, key):
    """(builder name, *arguments): built once per process."""
    if key not in _scenes:
        _scenes[key] = BUILDERS[key[0]](oracle, *key[1:])
    return _scenes[key]


def reference(oracle, sc, eps, kappa, ref_n=REF_N):
    """The model's plan, the oracle's radiance over its kept sets and the checked pixels, once per (scene, settings)."""
    key = ("_ref", eps, kappa, ref_n)
    if key not in sc:
        p = plan(sc, eps, kappa, ref_n)
        rad, img = oracle_radiance(oracle, sc, p)
        sc[key] = (p, rad, img, checked_pixels(p, rad))
    return sc[key]


EDGE_CASES = [("edge", k, side, pos) for k in (1, 2, 3, 5) for side in (-1, 1) for pos in ("first", "middle", "last")]
INST_CASES = [("inst", n, "last") for n in range(1, 18)] + [("inst", n, "first") for n in (9, 12, 13, 16)]
RAGGED_CASES = [("ragged", kind) for kind in ("narrow", "cross", "both")]
TIE_CASES = [("ties", copies, fit) for copies in (2, 3) for fit in (True, False)]
# one of each family at the library's default cull_eps, judged by statistics only (the scene is built for that eps: e / eps is the same)
DEFAULT_EPS_CASES = [("edge", 3, 1, "middle", EPS_DEFAULT), ("inst", 9, "last", EPS_DEFAULT), ("ragged", "both", EPS_DEFAULT),
                     ("ties", 3, False, EPS_DEFAULT), ("nothing", "one-lane", EPS_DEFAULT), ("lane", EPS_DEFAULT), ("factors", "plain", EPS_DEFAULT)]
AMBIGUOUS_MAX = 0.05     # of the image's rays, family 3 only


def case(key, eps=EPS_TEST, kappa=KAPPA, radiance=True):
    """One frame of the GPU suite: the scene, its settings, and what is asked of it.  exact: the model has no ambiguous ray, so the
    statistics must be EQUAL to its counts (every family but 3); marked: prune-on must differ from prune-off by at least half of
    what the oracle says the dropped set is worth (families 1, 2 and 4 at EPS_TEST, where something is dropped)."""
    name = "-".join(str(k) for k in key if k != eps) + ("" if kappa == KAPPA else f"-kappa{kappa:g}")
    return Scene(key=key, name=name, eps=eps, kappa=kappa, radiance=radiance and eps == EPS_TEST, exact=key[0] != "ragged",
                 marked=key[0] in ("edge", "inst", "ties") and eps == EPS_TEST and kappa > 0
                 and not (key[0] == "inst" and key[1] > PRUNE_PL) and not (key[0] == "edge" and key[1] == 1 and key[2] > 0))


CASES = ([case(k) for k in EDGE_CASES + INST_CASES + RAGGED_CASES + TIE_CASES + [("nothing", "none"), ("nothing", "one-lane")]]
         + [case(("lane",), kappa=0.0)]
         + [case(("factors", "plain"), kappa=k) for k in FACTOR_DROPS]
         + [case(("factors", kind)) for kind in ("albedo4", "negative", "large")]
         + [case(("factors", "albedo-inf"), radiance=False), case(("floor",), eps=1e-38, radiance=False)]
         + [case(k, eps=EPS_DEFAULT, kappa=0.0 if k[0] == "lane" else KAPPA) for k in DEFAULT_EPS_CASES])
