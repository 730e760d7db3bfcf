"""Scenes for the table kernel (csrc/vrt_table_kernel.hip) and a float64 model of the decisions it takes per 8x8 block: the menu of
table sizes, the segment count, which (wave, absorber) visits are settled by one add, and a ceiling of its own error bound.
tests/table_cases.py renders the cases on the GPU (tests/test_gpu_table.py), tests/test_table_scenes.py checks on the CPU that the
cases sit where they are meant to sit and can see what they are meant to see.  numpy and the oracle only: no GPU, no product import.

The kernel is compiled in two shapes, TableCfg<DW> for DW = 16 and 8 waves per block: tables of GMAX = 24 DW nodes (384 / 192),
segments of at most GMAX - 8 intervals (376 / 184), absorbers staged STAGE = 8 DW at a time (128 / 64), survivors gathered 64 DW at
a time (1024 / 512).  Per block it plans, from the block's longest sample range and its narrowest Gaussian,
    need = ceil(range r_max / hx)   intervals;   declined at need >= 8 (GMAX - 8)
    nseg = ceil(need / (GMAX - 8)), NT = the smallest of {4, 6, 8, 12, 16, 20, 24} with NT DW >= ceil(need / nseg) + 8
    SL = NT DW - 8 intervals per segment, the spacing reduced until nseg SL intervals cover the range exactly
so with every Gaussian of a scene in every block, a menu position is reached by the step hx alone.
"""
import math

import numpy as np

import boundary_scenes as B
from boundary_scenes import MARKER_FACTOR, PL, TOL, Scene, all_rays_see_all, marker_effects, marker_indices  # noqa: F401 (re-exported)

EXP_LIBM, EXP_VCL, EXP_FAST, EXP_SPLINE = 0, 1, 2, 3          # oracle/oracle.py and include/vrt_hip.h use the same numbers
ERF_LIBM, ERF_AS, ERF_SPLINE = 0, 1, 2
NT_MENU = (4, 6, 8, 12, 16, 20, 24)
TB_W0, TB_COUT = 0.0212, 0.36                                  # kink and smooth part of the interpolation error (kernel header)
U_MAX = 0.3                                                    # ... which hold for node spacings up to this, in units of 1/r
STEP_DEFAULT, BUDGET_DEFAULT, NOISE = 0.05, 2.5e-5, 5e-6       # library defaults; fp32 noise of two summation orders (test_gpu_parity)
ADAPT_DEFAULT = 3.0                                            # VRT_HIP_TABLE_ADAPT: the first attempt may be this much coarser
SQRT_2PI = 2.5066282746310002


def gmax(dw): return 24 * dw
def stage(dw): return 8 * dw
def seg_max(dw): return gmax(dw) - 8                           # intervals of the longest segment
def need_limit(dw): return 8 * seg_max(dw)                     # declined from here on
def table_saturation(erf_kind): return 4.5 if erf_kind == ERF_AS else 3.5
def table_saturation_eps(erf_kind): return 1.25 * 4.31e-7 if erf_kind == ERF_AS else 1.25 * 7.44e-7


# ---- the plan ----
def plan_of_need(need, dw):
    """(nseg, NT) for `need` intervals, None where the kernel declines."""
    need = max(int(need), 0)
    if need >= need_limit(dw):
        return None
    nseg = max(1, -(-need // seg_max(dw)))
    sl_need = max(1, -(-need // nseg))
    nt = -(-(sl_need + 8) // dw)
    return nseg, next((m for m in NT_MENU if nt <= m), NT_MENU[-1])


def need_of(range_, r_max, hx):
    return int(math.ceil(range_ * r_max / hx))


def plan(range_, r_max, hx, dw):
    """The `plan` lambda of render_table_body in float64: (nseg, NT, SL, G, Gtot, h, u), or None where the kernel declines (more
    than eight segments, or a spacing beyond 0.3 / r_max that the menu cannot reduce)."""
    p = plan_of_need(need_of(range_, r_max, hx), dw)
    if p is None:
        return None
    nseg, nt = p
    g = nt * dw
    sl = g - 8
    ht = hx / r_max
    h = min(ht, range_ / (nseg * sl) * 1.00001)
    if not h > 0.0:
        h = ht
    u = h * r_max
    return None if u > U_MAX else (nseg, nt, sl, g, nseg * sl + 6, h, u)


def margin_of_need(need, dw, cap=64):
    """By how many intervals `need` may move either way without changing (nseg, NT) or crossing the decline limit."""
    here = plan_of_need(need, dw)
    for d in range(1, cap + 1):
        if plan_of_need(need + d, dw) != here or plan_of_need(need - d, dw) != here:
            return d - 1
    return cap


def bands(dw):
    """[(NT, smallest need, largest need)] of the one-segment plans."""
    out, lo = [], 0
    for nt in NT_MENU:
        out.append((nt, lo, nt * dw - 8))
        lo = nt * dw - 8 + 1
    return out


# ---- a scene as the kernel sees it, in float64 ----
def _geometry(sc):
    if "_geom" in sc:
        return sc["_geom"]
    o = sc.origin.astype(np.float64)
    d = np.stack([np.asarray(a, np.float64) for a in sc.plane], 1) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    oc = sc.g["mu"][:, :3].astype(np.float64) - o
    mubar = d @ oc.T                                                            # [ray, gaussian]
    d2 = np.maximum((oc * oc).sum(1)[None, :] - mubar * mubar, 0.0)
    s32 = sc.g["sigma"].astype(np.float32)
    r = (np.float32(1.0) / (np.float32(1.41421356237309504880) * s32)).astype(np.float64)   # gB.x, build_static_kernel
    sigma, mag = s32.astype(np.float64), sc.g["magnitude"].astype(np.float64)
    A = (sigma * mag / SQRT_2PI)[None, :] * np.exp(-d2 / (2.0 * sigma * sigma)[None, :])     # gB.z Exp(-d2 gB.y)
    blocks = [np.array([(by * 8 + iy) * sc.w + bx * 8 + ix for iy in range(8) for ix in range(8)])
              for by in range(sc.h // 8) for bx in range(sc.w // 8)]
    s_lo = (mubar - 2.8285 / r[None, :]).min(1)                                 # per ray: the first sample the table must cover
    s_hi = mubar.max(1)
    sc["_geom"] = Scene(mubar=mubar, d2=d2, r=r, sigma=sigma, mag=mag, A=A, blocks=blocks, s_lo=s_lo, s_hi=s_hi)
    return sc["_geom"]


def block_ranges(sc):
    """Per 8x8 block of the image: ([range], [r_max]) -- the longest sample range of the block's rays,
    max_j mubar_j - min_j (mubar_j - 2.8285 / r_j), and the largest r_j = 1 / (sqrt2 sigma_j) as the kernel reads it (float32)."""
    G = _geometry(sc)
    return (np.array([(G.s_hi[b] - G.s_lo[b]).max() for b in G.blocks]), np.full(len(G.blocks), G.r.max()))


def block_needs(sc, hx):
    rng, rmax = block_ranges(sc)
    return [need_of(a, b, hx) for a, b in zip(rng, rmax)]


def block_plans(sc, hx, dw):
    rng, rmax = block_ranges(sc)
    return [plan(a, b, hx, dw) for a, b in zip(rng, rmax)]


def expected_nodes(sc, hx, dw):
    """What vrt_hip_stats.table_nodes must read: the sum of Gtot over the blocks the kernel keeps."""
    return sum(p[4] for p in block_plans(sc, hx, dw) if p is not None)


def menu_margin(sc, hx, dw):
    """The distance, in intervals, of the blocks' `need` from the nearest edge of the menu (an NT threshold, a segment-count
    threshold, the decline limit): the smallest over the blocks."""
    return min(margin_of_need(n, dw) for n in block_needs(sc, hx))


def step_for(sc, need, which):
    """The step at which the block with the smallest (`min`) or the largest (`max`) range needs `need` intervals (in the middle of
    the ceil's unit interval)."""
    rng, rmax = block_ranges(sc)
    R = rng * rmax
    return float((R.min() if which == "min" else R.max()) / (need - 0.5))


def bound_ceiling(sc, hx, dw, erf_kind=ERF_AS, adapt=1.0):
    """An upper bound of the kernel's own per-ray bound, from the scene alone: the formula of the kernel's header comment with every
    weight at its worst, K(g) <= S_all and s3 <= 255:  1.01 S_max (0.0212 u^2 + 0.36 u^4 + table_saturation_eps) L_max,
    S_max = the largest sum_j |A_j| of a ray, L_max = the largest sum_ik amax_i |term_ik| of a ray with the transmittance at 1.
    A budget of this size keeps every block on its first attempt whatever the kernel does inside.  adapt > 1: for a context that
    may coarsen the requested spacing by up to that factor on its first attempt (u <= min(0.3, adapt hx) then)."""
    G = _geometry(sc)
    us = [p[6] for p in block_plans(sc, hx, dw) if p is not None]
    if not us:
        return 0.0
    u = max(us) if adapt <= 1.0 else max(max(us), min(U_MAX, adapt * hx))
    S_max = np.abs(G.A).sum(1).max()
    amax = np.abs(sc.g["albedo"].astype(np.float64)).max(1)
    q = np.abs(G.sigma * G.mag)
    k2 = np.arange(-4, 1, dtype=np.float64) ** 2
    L = ((amax * q * np.exp(-k2 / 2.0).sum())[None, :] * np.exp(-G.d2 / (2.0 * G.sigma ** 2)[None, :])).sum(1)
    return float(1.01 * S_max * (TB_W0 * u * u + TB_COUT * u ** 4 + table_saturation_eps(erf_kind)) * L.max())


def budget_of(sc, hx, dw, erf_kind=ERF_AS):
    """The budget a case renders with: the default where the ceiling fits it, the ceiling otherwise."""
    return max(BUDGET_DEFAULT, bound_ceiling(sc, hx, dw, erf_kind))


def skip_bounds(sc, hx, dw, erf_kind=ERF_AS):
    """(lower, upper) for vrt_hip_stats.table_skips: the (block, segment, wave, absorber) visits whose Erf argument lies beyond the
    saturation point (+ 1e-3) on all of the wave's nodes and all 64 rays, x_hi <= -sat or x_lo >= sat with
    x = c + g h r, c = s_seg r - m between its smallest and largest value over the block's rays -- counted with a margin of 1e-2
    against the fp32 rounding of the kernel's arguments: visits that hold by that margin, and visits that hold up to it."""
    G = _geometry(sc)
    sat = table_saturation(erf_kind) + 1e-3
    lower = upper = 0
    for b, p in zip(G.blocks, block_plans(sc, hx, dw)):
        if p is None:
            continue
        nseg, nt, sl, _, _, h, _ = p
        lo = G.s_lo[b] - 2.0 * h                                                # per ray: node 0 of its grid
        for seg in range(nseg):
            s_seg = lo + (seg * sl - 2.0) * h
            c = s_seg[:, None] * G.r[None, :] - G.mubar[b] * G.r[None, :]
            cmin, cmax = c.min(0), c.max(0)
            for wave in range(dw):
                x_lo = wave * nt * h * G.r + cmin
                x_hi = (wave * nt + nt - 1) * h * G.r + cmax
                lower += int((x_hi <= -(sat + 1e-2)).sum() + (x_lo >= sat + 1e-2).sum())
                upper += int((x_hi <= -(sat - 1e-2)).sum() + (x_lo >= sat - 1e-2).sum())
    return lower, upper


def _block_of_pixel(sc, pix):
    return (int(pix) // sc.w // 8) * (sc.w // 8) + (int(pix) % sc.w) // 8


def grid_positions(sc, hx, dw, s, pix):
    """Positions on the node grid of the ray of pixel `pix` (node 0 = two nodes before its first sample) of the ray parameters
    `s`, with the plan of the pixel's block; and that plan."""
    G = _geometry(sc)
    p = block_plans(sc, hx, dw)[_block_of_pixel(sc, pix)]
    return (np.asarray(s, np.float64) - (G.s_lo[pix] - 2.0 * p[5])) / p[5], p


def straddlers(sc, hx, dw):
    """For a multi-segment case, on every checked pixel: (the markers whose five samples as EMITTERS fall into two different
    segments, the markers whose kink as ABSORBERS lies within one interval of a segment border)."""
    G = _geometry(sc)
    emit, kink = set(sc.markers), set(sc.markers)
    for pix in sc.pixels:
        for k in sc.markers:
            s = G.mubar[pix, k] + np.arange(-4, 1) * G.sigma[k]
            pos, p = grid_positions(sc, hx, dw, s, pix)
            nseg, _, sl, _, gtot = p[:5]
            gi = np.clip(np.floor(pos), 2, gtot - 4)
            if len(set(np.minimum(gi // sl, nseg - 1))) < 2:
                emit.discard(k)
            if not any(abs(pos[4] - border * sl) <= 1.0 for border in range(1, nseg)):
                kink.discard(k)
    return sorted(emit), sorted(kink)


# ---- scenes ----
FOCAL = 12.0  # a narrow image (+-5 degrees): every ray still sees the whole of a Gaussian 40 sigma behind the first.  The reference's tile
              # rule keeps what lies at least focal + 1 in front of the camera


def depth_stack(oracle, n, depth, sigma, t0, marker_t=None, tau_cloud=0.6, tau_marker=0.4, w=16, h=16, seed=0, threads=8):
    """n Gaussians along the view axis, their centres between t0 and t0 + depth from the camera, all about `sigma` wide
    (sigma .. 1.15 sigma, the markers sigma: r_max is the markers'), within 0.3 sigma of the axis; one tile, every ray of the
    16x16 image sees all of them with cull_eps = 0.  The first and the last in depth are ordinary members of the cloud ON the axis:
    the sample range does not depend on where the markers are.  Markers (marker_indices(PL, n): the ends of the list and both sides
    of the hand-over limit) are on the axis at the distances `marker_t` (default: spread over the depth), strong (optical depth
    tau_marker each against tau_cloud for the whole cloud) and each of a colour of its own.  Depth order is not list order.
    Checked pixels: the one on the axis and two of its neighbours, in three different blocks."""
    rng = np.random.default_rng(4000 + 16 * n + seed)
    cam, _ = oracle.cli_camera(w, h, focal=FOCAL)
    plane, view, origin = oracle.camera_plane(cam), oracle.camera_view(cam), np.array(cam.position[:], np.float32)
    markers = marker_indices(PL, n)
    others = [i for i in range(n) if i not in markers]
    t = np.zeros(n)
    mu = np.zeros((n, 3))
    tt = t0 + depth * np.linspace(0.0, 1.0, len(others))
    order = rng.permutation(len(others))
    sig = rng.uniform(sigma, 1.15 * sigma, n)
    for rank, i in enumerate(np.asarray(others)[order]):
        t[i] = tt[rank]
        mu[i, :2] = 0.0 if rank in (0, len(others) - 1) else rng.normal(size=2) * 0.3 * sigma
    sig[np.asarray(others)[order][0]] = 1.15 * sigma                            # the first sample of every ray: t0 - 4.6 sigma
    if marker_t is None:
        marker_t = t0 + depth * (np.arange(len(markers)) + 0.5) / len(markers)
    tau = rng.uniform(0.5, 1.5, n) * tau_cloud / len(others)
    alb = rng.uniform(0.1, 1.0, size=(n, 4))
    for j, k in enumerate(markers):
        t[k], sig[k], tau[k] = marker_t[j], sigma, tau_marker
        alb[k] = [(1.0, 0.3, 0.2, 1.0), (0.2, 1.0, 0.3, 1.0), (0.3, 0.2, 1.0, 1.0), (1.0, 1.0, 0.2, 1.0)][j % 4]
    mu[:, 2] = origin[2] + t                                                    # the CLI camera looks along +z
    g = oracle.gaussians(alb, mu, sig, tau / (SQRT_2PI * sig))
    tiles = oracle.tile_gaussians(2.0, 2.0, g, view)
    assert tiles["w"] == tiles["h"] == 1 and tiles["offsets"][1] == n
    axis = (h // 2) * w + w // 2
    return Scene(g=g, n=n, cap=PL, w=w, h=h, tw=2.0, th=2.0, plane=plane, view=view, origin=origin, tiles=tiles, markers=markers,
                 pixels=np.array([axis - w - 1, axis - 1, axis], np.uint32), marker_t=np.asarray(marker_t, np.float64))


SIGMA = 1.0
SHALLOW = dict(n=40, depth=SIGMA, sigma=SIGMA, t0=20.0)         # range r_max ~ 4: NT = 4 at u <= 0.3 even for 8 waves (SL = 24)
DEEP = dict(n=48, depth=42.0, sigma=SIGMA, t0=18.0)             # range r_max ~ 33: eight segments and the decline limit at hx >= 0.01


def shallow_stack(oracle):
    return depth_stack(oracle, **SHALLOW)


def deep_stack(oracle, need=None, which="min", dw=16):
    """The deep stack; with `need`: the markers placed for the step that gives that need -- marker 0 half an interval behind the
    first segment border of the axis ray (its kink within one interval of the border, its last sample beyond it and the other
    four before), marker 1 half an interval before the last border, the others where they were."""
    sc = depth_stack(oracle, **DEEP)
    if need is None:
        return sc
    hx = step_for(sc, need, which)
    axis = int(sc.pixels[-1])
    _, p = grid_positions(sc, hx, dw, [0.0], axis)
    nseg, _, sl, _, _, h, _ = p
    lo = _geometry(sc).s_lo[axis] - 2.0 * h
    mt = sc.marker_t.copy()
    mt[0] = lo + (sl + 0.5) * h
    mt[1] = lo + ((nseg - 1) * sl - 0.5) * h
    out = depth_stack(oracle, marker_t=mt, **DEEP)
    assert np.allclose(block_ranges(out)[0], block_ranges(sc)[0], rtol=0, atol=1e-12)   # the markers are inside the range
    return out
