"""Scenes for the list kernels (csrc/vrt_kernels.hip: build_tile_lists_body with its phases chunk_test, filter_cells, file_cells and
clear_empty_cells; the unfused pair build_tile_lists_kernel + build_cell_lists_kernel; the cone table) and a float64 model of what
they decide: per tile the length of its work list, per 32x32 cell the length of its list (or the overflow mark), the class it is
filed as and the length a block of it starts from.  tests/test_gpu_lists.py renders them on the GPU, tests/test_list_scenes.py checks
on the CPU that they can see what they are meant to see.  numpy and the oracle only: no GPU, no product import.

What the code decides.  Thresholds are in x = d^2 / (2 sigma^2); cull_x, its error and the Exp floor are block_scenes.geometry's.
  tile   a Gaussian enters the tile's work list iff it is in the tile's given list -- the reference's tile test for device binning
         (taken from oracle.tile_gaussians, which is the device's set bit for bit: tests/test_gpu_parity.py), a caller's list, or every
         index when there are no tiles -- AND cone_keeps(tile cone, cull_x), no slack.  total = the length of the list.
  cell   32x32 pixels, clipped to the tile; cells_x = ceil(tile_w / 32), cell ci at (ci % cells_x, ci / cells_x).  A Gaussian of the
         tile's list enters iff cone_keeps(cell cone, cull_x - ln(ref_n / max(total, 1))); no slack at the Exp floor or with ref_n = 0.
         fused kernel (at most 64 cells per tile): total > TCAP = 1024 gives every cell of the tile the mark 0xFFFFFFFF -- its blocks
         read the tile's list, it is filed as dense, n_list = total, whatever its own cone would have kept.  Either kernel: a cell
         with more than cstride = min(N, 4096) entries gets the mark too.  The unfused kernel has no TCAP, so total may exceed ref_n
         (1365.33): the slack is then negative and the threshold rises.
  no refine  (row stride tile_w tiles_w != image width, or a plane that is no pinhole pattern) both levels keep what they are given.
  filing     empty | light (count <= 24, fused raster frames only) | active | dense (count > 96, or the mark).
A cone is rect_cone over the rectangle's pixels: axis = the ray of pixel ((x0 + x1 + 1) / 2, (y0 + y1 + 1) / 2), cosine and sine from the
four corner rays, make_cone's 0.9999 / 1.001 + 1e-6, then + 1e-4 on the sine.  block_scenes._rect_cone restates it; a tile's rectangle
is given to it in image coordinates (refine implies that the tile is a rectangle of the image, and the centre pixel of a shifted
rectangle is the shifted centre pixel).

The margin of a cone decision is block_scenes._cone_keeps' (derived there for the block cone, whose axis is normalised with the
hardware reciprocal square root as well) plus one term.  The list kernels' cones are built from cone_ray's directions: n' = (p - o)
rsq(|p - o|^2), where the block cone's rays are exactly normalised.  The squared norm carries 3 roundings (relative 3 2^-24, halved by
the root), v_rsq_f32 is good to 1 ulp (2^-23) and each product with it rounds once more (2^-24): every component of n' is within
2^-22 |n| of n.  The cosine n_k . n_c of two such vectors is then off by at most 2 2^-22 plus its own three roundings (3 2^-24):
below 2^-21 = ERR_RSQ.  The sine |n_k x n_c| likewise: each component of the cross product is a difference of two products of size <=
1 (2 2^-24 from their roundings, 4 2^-24 from the inputs), the root is 1 ulp: below 2^-21 absolute for the cones here (sin < 0.5).
make_cone's factors are restated, so the model's cone differs from the device's by d cos, d sin <= ERR_RSQ, and dmin = dperp cos - |tc|
sin by at most ERR_RSQ (dperp + |tc|); with v = 0.999 dmin^2 / (2 sigma^2) that is dv <= 2 dmin ERR_RSQ (dperp + |tc|) / (2 sigma^2),
the term _cone_keeps adds with rsq=True.  It is 1.4e-3 for sigma = 0.01 at v = 100 and |oc| = 5, below the margin's other terms.
No margin is tuned on the GPU.

A cloud is drawn from a seed; `settle` then plans every frame the suites make of it, removes every Gaussian that is inside the margin
of any cone decision of any of them, and plans again until none is left: the GPU tests assert EQUAL counts, not brackets.
"""
import numpy as np

from block_scenes import EPS_DEFAULT, EPS_TEST, PL, REF_N, Scene, _cone_keeps, _rect_cone, _slack, _threshold, geometry
from boundary_scenes import CSTRIDE_MAX, LIGHT_CELLS, MAX_FUSED_CELLS, PCAP, TCAP, TOL  # noqa: F401 (TOL re-exported)

CELL, BLOCK = 32, 8
MARK = 0xFFFFFFFF
EMPTY, LIGHT, ACTIVE, DENSE = "empty", "light", "active", "dense"
EXP_FLOOR = {"vcl": float(np.float32(87.3)), "libm": 104.0}          # exp_floor_x (csrc/vrt_hip_api.cpp)
REMOVED_MAX = 0.05
# wrong variants of the model: switches of plan_lists, for tests/test_list_scenes.py
WRONG = ("no-slack", "slack-from-n", "cell-not-clipped", "no-tcap", "tcap-unfused", "ci-by-cells_y", "tile-by-tiles_h", "sine-tight",
         "sine-doubled", "eps-without-n")


# ---- geometry of tiles, cells and blocks ----
def grid(sc, mode="device"):
    """tile_geometry and the cell grid (csrc/vrt_hip_api.cpp, vrt_hip_frame.cpp: plan_lists), in the host's fp32 steps."""
    f = np.float32
    if mode == "none":
        tiles_w = tiles_h = 1
        tile_w, tile_h = sc.w, sc.h
    else:
        tiles_w, tiles_h = int(np.ceil(f(2.0) / f(sc.tw))), int(np.ceil(f(2.0) / f(sc.th)))
        tile_w, tile_h = int(f(sc.w) * f(sc.tw) / f(2.0)), int(f(sc.h) * f(sc.th) / f(2.0))
    cells_x, cells_y = -(-tile_w // CELL), -(-tile_h // CELL)
    return Scene(tiles_w=tiles_w, tiles_h=tiles_h, n_tiles=tiles_w * tiles_h, tile_w=tile_w, tile_h=tile_h, stride=tile_w * tiles_w,
                 cells_x=cells_x, cells_y=cells_y, cpt=cells_x * cells_y, npix=sc.w * sc.h, refine=tile_w * tiles_w == sc.w)


def inside_blocks(L, ci):
    """How many of the 16 blocks of cell ci lie inside the tile (block_of(...).inside: the block's first pixel is a pixel of the tile)."""
    cxi, cyi = ci % L.cells_x, ci // L.cells_x
    return sum(1 for bi in range(16) if (cxi * 4 + (bi & 3)) * BLOCK < L.tile_w and (cyi * 4 + (bi >> 2)) * BLOCK < L.tile_h)


def cell_lanes(L, t, ci):
    """Per inside block of cell ci of tile t: (the raster pixel whose ray each of the 64 lanes takes, which lanes write)."""
    tx, ty = t % L.tiles_w, t // L.tiles_w
    cxi, cyi = ci % L.cells_x, ci // L.cells_x
    lane = np.arange(64)
    out = []
    for bi in range(16):
        bx, by = cxi * 4 + (bi & 3), cyi * 4 + (bi >> 2)
        if not (bx * BLOCK < L.tile_w and by * BLOCK < L.tile_h):
            continue
        pxt, pyt = bx * BLOCK + (lane & 7), by * BLOCK + (lane >> 3)
        valid = (pxt < L.tile_w) & (pyt < L.tile_h)
        pix = tx * L.tile_w + np.minimum(pxt, L.tile_w - 1) + L.stride * (ty * L.tile_h + np.minimum(pyt, L.tile_h - 1))
        valid &= pix < L.npix
        out.append((np.minimum(pix, L.npix - 1), valid))
    return out


def cell_pixels(L, key):
    """The raster pixels that cell `key` = tile * cells per tile + ci owns."""
    return np.concatenate([pix[valid] for pix, valid in cell_lanes(L, key // L.cpt, key % L.cpt)])


def tile_lists(ref):
    """oracle.tile_gaussians' result as one index array per tile."""
    off = ref["offsets"]
    return [np.asarray(ref["indices"][off[t]:off[t + 1]], np.int64) for t in range(int(ref["w"]) * int(ref["h"]))]


# ---- the model ----
def _variant_cone(cone, wrong):
    axis, cos_t, sin_t = cone
    if wrong == "sine-tight":
        sin_t = (sin_t - 1e-4 - 1e-6) / 1.001 + 1e-6
    if wrong == "sine-doubled":
        sin_t = 2.0 * sin_t
    return axis, cos_t, sin_t


def _cell_class(count, light):
    if count == 0:
        return EMPTY
    if count > PCAP:
        return DENSE
    return LIGHT if light and count <= LIGHT_CELLS else ACTIVE


def plan_lists(sc, eps=EPS_DEFAULT, ref_n=REF_N, fused=None, refine=None, light=True, mode="device", lists=None, exp="vcl", wrong=None):
    """The model's lists for one frame of view `sc`.  mode: "device" (the reference's tile sets), "lists" (caller-made: `lists`, one
    index array per tile; default the reference's) or "none" (no tiles: one tile, every index).  fused / refine: which kernel and
    whether it culls; default what the host would choose (vrt_hip_frame.cpp: plan_lists).  light: a raster frame (light filing on where
    fused).  Returns per tile `total`, per cell count | MARK, class, n_list and inside blocks, and what the suites derive from them."""
    key = ("_lists", eps, ref_n, fused, refine, light, mode, None if lists is None else tuple(map(len, lists)), exp, wrong)
    if key in sc and lists is None:
        return sc[key]
    L = grid(sc, mode)
    refine = L.refine if refine is None else refine
    fused = (L.cpt <= MAX_FUSED_CELLS and (mode == "device" or refine)) if fused is None else fused
    floor = EXP_FLOOR[exp]
    G = geometry(sc, eps, floor=floor, rays=False, scale_n=wrong != "eps-without-n")
    n = len(sc.g)
    cstride = max(1, min(n, CSTRIDE_MAX))
    given = [np.arange(n)] if mode == "none" else (tile_lists(sc.ref) if lists is None else [np.asarray(l, np.int64) for l in lists])
    assert len(given) == L.n_tiles, (len(given), L.n_tiles)
    thr0 = _threshold(G, 0.0)
    unsure = set()
    totals, cells = [], []
    slack_min = np.inf
    for t in range(L.n_tiles):
        tx, ty = (t % L.tiles_h, t // L.tiles_h) if wrong == "tile-by-tiles_h" else (t % L.tiles_w, t // L.tiles_w)
        ox, oy = tx * L.tile_w, ty * L.tile_h
        members = given[t]
        if refine and len(members):
            cone = _variant_cone(_rect_cone(sc, G, ox, oy, ox + L.tile_w - 1, oy + L.tile_h - 1), wrong)
            keep, sure = _cone_keeps(G, cone, thr0, members, rsq=True)
            unsure |= set(members[~sure].tolist())
            members = members[keep]
        total = len(members)
        totals.append(total)
        slack = 0.0 if wrong == "no-slack" else _slack(ref_n, n if wrong == "slack-from-n" else total)
        if total:
            slack_min = min(slack_min, slack)
        thr = _threshold(G, slack)
        over_tcap = total > TCAP and (fused or wrong == "tcap-unfused") and wrong != "no-tcap"
        for ci in range(L.cpt):
            cxi, cyi = (ci % L.cells_y, ci // L.cells_y) if wrong == "ci-by-cells_y" else (ci % L.cells_x, ci // L.cells_x)
            kept = members
            if over_tcap:
                count = MARK
            elif refine and total:
                x0, y0 = cxi * CELL, cyi * CELL
                x1, y1 = (x0 + CELL - 1, y0 + CELL - 1) if wrong == "cell-not-clipped" else (min(x0 + CELL, L.tile_w) - 1, min(y0 + CELL, L.tile_h) - 1)
                cone = _variant_cone(_rect_cone(sc, G, ox + x0, oy + y0, ox + x1, oy + y1), wrong)
                keep, sure = _cone_keeps(G, cone, thr, members, rsq=True)
                unsure |= set(members[~sure].tolist())
                kept = members[keep]
                count = len(kept)
            else:
                count = total
            cls = _cell_class(count, light and fused)       # (the unfused kernel classes by the count itself: beyond cstride that is dense too)
            if count != MARK and count > cstride:
                count = MARK
            cells.append(Scene(tile=t, ci=ci, key=t * L.cpt + ci, count=count, cls=cls, n_list=total if count == MARK else count,
                               inside=inside_blocks(L, ci), kept=kept))
    lit = [c for c in cells if c.count]
    dense_lo, dense_exact = sum(c.inside for c in lit if c.cls == DENSE), True
    for c in lit:       # a block of a cell that is not dense goes to the dense path iff a ray of it keeps more than PL: decided from x <= cull_x + margin,
        if c.cls == DENSE or c.n_list <= PL:        # an upper bound of what the ray keeps (the lane's slack is positive: its block has at most 96 survivors)
            continue
        j = c.kept
        for pix, _ in cell_lanes(L, c.tile, c.ci):
            mubar = G.d[pix] @ G.oc[j].T
            x = np.maximum(G.w2[j][None, :] - mubar * mubar, 0.0) * G.inv2s2[j][None, :]
            err = (16 * 2.0 ** -24 * G.w2[j] * G.inv2s2[j])[None, :] + 2.0 ** -22 * x + G.err_cull[j][None, :]
            if (x <= G.cull_x[j][None, :] + err).sum(1).max() > PL:
                dense_exact = False
    p = Scene(L=L, fused=fused, refine=refine, totals=totals, cells=cells, unsure=len(unsure), unsure_idx=unsure, slack_min=slack_min,
              cells_lit={c.key for c in lit}, shaded_blocks=sum(c.inside for c in lit), tile_entries=sum(c.n_list * c.inside for c in lit),
              dense_blocks=dense_lo, dense_exact=dense_exact, classes={k: sum(1 for c in cells if c.cls == k) for k in (EMPTY, LIGHT, ACTIVE, DENSE)},
              marked=sum(1 for c in cells if c.count == MARK))
    if lists is None:
        sc[key] = p
    return p


def observables(p):
    return p.cells_lit, p.shaded_blocks, p.tile_entries


# ---- clouds, views and frames ----
def _cam(oracle, w, h, rot=0.0):
    cam, _ = oracle.cli_camera(w, h, initial_rot=rot)
    return oracle.camera_plane(cam), oracle.camera_view(cam), np.array(cam.position[:], np.float32)


def at_image(oracle, u, v, depth):
    """World points that the unrotated camera sees at the image position (u, v) in [0, 1)^2, `depth` plane distances away."""
    plane, _, origin = _cam(oracle, 64, 64)
    p = np.stack([np.asarray(a, np.float64) for a in plane], 1).reshape(64, 64, 3)
    ex, ey = (p[0, 63] - p[0, 0]) / 63.0, (p[63, 0] - p[0, 0]) / 63.0
    pp = p[0, 0][None, :] + 64.0 * np.asarray(u)[:, None] * ex[None, :] + 64.0 * np.asarray(v)[:, None] * ey[None, :]
    o = origin.astype(np.float64)
    return o[None, :] + (pp - o[None, :]) * np.asarray(depth)[:, None]


def view_of(oracle, cloud, view):
    """The cloud under view = (w, h, tiles per row, tiles per column, camera rotation in degrees): what plan_lists takes."""
    if view not in cloud.views:
        w, h, ntx, nty, rot = view
        plane, mat, origin = _cam(oracle, w, h, rot)
        tw, th = 2.0 / ntx, 2.0 / nty
        ref = oracle.tile_gaussians(tw, th, cloud.g, mat)
        assert (int(ref["w"]), int(ref["h"])) == (ntx, nty)
        cloud.views[view] = Scene(g=cloud.g, n=len(cloud.g), w=w, h=h, tw=tw, th=th, plane=plane, view=mat, origin=origin, ref=ref)
    return cloud.views[view]


def frame(view, mode="device", eps=EPS_DEFAULT, ref_n=REF_N, exp="vcl", chunks=False, name=None):
    """One frame of the suites: a view of a cloud and the settings it is rendered with."""
    w, h, ntx, nty, rot = view
    name = name or "-".join([f"{w}x{h}", f"{ntx}x{nty}" if mode != "none" else "untiled"] + ([f"rot{rot:g}"] if rot else []) + ([mode] if mode != "device" else [])
                            + ([f"eps{eps:g}"] if eps != EPS_DEFAULT else []) + (["ref_n0"] if ref_n == 0 else []) + ([exp] if exp != "vcl" else [])
                            + (["chunks"] if chunks else []))
    return Scene(view=view, mode=mode, eps=eps, ref_n=ref_n, exp=exp, chunks=chunks, name=name)


def frame_lists(oracle, cloud, fr):
    """The caller-made lists of a frame: the reference's, or ("lists-minus") those with the first Gaussian that the first lit cell of the
    longest list below TCAP keeps taken out of that tile's list by hand."""
    sc = view_of(oracle, cloud, fr.view)
    if fr.mode not in ("lists", "lists-minus"):
        return None
    lists = tile_lists(sc.ref)
    if fr.mode == "lists-minus":
        p = plan_lists(sc, fr.eps, fr.ref_n, light=True, mode="lists", exp=fr.exp)
        t = max((t for t in range(len(lists)) if p.totals[t] <= TCAP), key=lambda t: p.totals[t])
        victim = next(c for c in p.cells if c.tile == t and c.count).kept[0]
        lists[t] = lists[t][lists[t] != victim]
        fr["victim"] = (t, int(victim))
    return lists


def plan_frame(oracle, cloud, fr, light=True, wrong=None):
    sc = view_of(oracle, cloud, fr.view)
    mode = "lists" if fr.mode == "lists-minus" else fr.mode
    return plan_lists(sc, fr.eps, fr.ref_n, light=light, mode=mode, lists=frame_lists(oracle, cloud, fr), exp=fr.exp, wrong=wrong)


def settle(oracle, name, g, frames, rounds=8):
    """Remove what any frame's model is unsure of, until no frame is unsure of anything."""
    drawn = len(g)
    for _ in range(rounds):
        cloud = Scene(name=name, g=np.ascontiguousarray(g), views={}, drawn=drawn, removed=drawn - len(g), frames=frames)
        bad = set()
        for fr in frames:
            bad |= plan_frame(oracle, cloud, fr).unsure_idx
        if not bad:
            return cloud
        g = np.delete(g, sorted(bad))
    raise AssertionError(f"{name}: still unsure after {rounds} rounds")


def _draw(oracle, rng, u, v, sigma, depth=None, mag=None):
    n = len(u)
    depth = rng.uniform(4.7, 5.3, n) if depth is None else depth
    mu = at_image(oracle, u, v, depth)
    mag = rng.uniform(0.5, 2.0, n) if mag is None else mag
    return oracle.gaussians(rng.uniform(0.2, 1.0, size=(n, 4)), mu, sigma, mag)


GRID_VIEW, GRID_VIEW_B = (256, 256, 4, 4, 0.0), (256, 256, 4, 4, 14.0)
# The grid cloud is settled three times from the same draw, for the paths, the thresholds and the two cameras: what one frame's model is
# unsure of need not leave the scenes of the others
GRID_FRAMES = [frame(GRID_VIEW), frame(GRID_VIEW, mode="lists"), frame(GRID_VIEW, mode="lists-minus"), frame(GRID_VIEW, mode="none"),
               frame(GRID_VIEW, chunks=True)]
THRESHOLD_FRAMES = [frame(GRID_VIEW, eps=EPS_TEST), frame(GRID_VIEW, eps=0.0), frame(GRID_VIEW, eps=0.0, exp="libm"), frame(GRID_VIEW, ref_n=0.0)]
CAMERA_FRAMES = [frame(GRID_VIEW), frame(GRID_VIEW_B)]


def _grid_cloud(oracle, seed=11):
    """Family 1 (and 5, 7, 8): about 600 Gaussians, sigma 0.01 .. 0.05, for 256 x 256 pixels in 4 x 4 tiles of 2 x 2 cells: a tight
    cluster inside one cell (dense), a looser one around it and across a tile border (active), a thin spread over the right half
    (light), the lower left left empty; six Gaussians of magnitude 0 and six of negative magnitude among them."""
    rng = np.random.default_rng(seed)
    n1, n2, n3 = 140, 280, 180
    u = np.concatenate([rng.normal(0.3125, 0.018, n1), rng.normal(0.40, 0.09, n2), rng.uniform(0.5, 1.0, n3)])
    v = np.concatenate([rng.normal(0.3125, 0.018, n1), rng.normal(0.36, 0.09, n2), rng.uniform(0.0, 1.0, n3)])
    g = _draw(oracle, rng, np.clip(u, 0.01, 0.99), np.clip(v, 0.01, 0.99), rng.uniform(0.01, 0.05, n1 + n2 + n3))
    g = g[rng.permutation(len(g))]          # scene order shuffled: a chunk of 64 consecutive indices spans the scene
    special = rng.choice(len(g), 12, replace=False)
    g["magnitude"][special[:6]] = 0.0
    g["magnitude"][special[6:]] *= -1.0
    return g


def _uniform_cloud(oracle, seed, n, s_lo, s_hi, box=(0.02, 0.98, 0.02, 0.98)):
    rng = np.random.default_rng(seed)
    return _draw(oracle, rng, rng.uniform(box[0], box[1], n), rng.uniform(box[2], box[3], n), rng.uniform(s_lo, s_hi, n))


NARROW_FUSED, NARROW_PAIR, NARROW_ONE = (128, 128, 2, 2, 0.0), (576, 272, 2, 1, 0.0), (256, 288, 1, 1, 0.0)


def _narrow_cloud(oracle, seed=23):
    """Families 3 and 4: 2500 narrow Gaussians (sigma 0.01 .. 0.03), 1200 of them in the upper left quadrant, 100 in the lower left,
    600 in each quadrant on the right.  As 2 x 2 tiles of 64 pixels (fused) the upper left tile is beyond TCAP and its neighbours are
    not; as 2 x 1 tiles of 288 x 272 pixels (81 cells: unfused) the left tile holds about 1300 -- beyond TCAP, which must not matter
    there, and below ref_n --; as one tile of 256 x 288 pixels (72 cells) the list is beyond ref_n = 1365.33 and the cell slack negative."""
    rng = np.random.default_rng(seed)
    quad = [(0.02, 0.48, 0.02, 0.48, 1200), (0.02, 0.48, 0.52, 0.98, 100), (0.52, 0.98, 0.02, 0.48, 600), (0.52, 0.98, 0.52, 0.98, 600)]
    u = np.concatenate([rng.uniform(a, b, k) for a, b, _, _, k in quad])
    v = np.concatenate([rng.uniform(c, d, k) for _, _, c, d, k in quad])
    g = _draw(oracle, rng, u, v, rng.uniform(0.01, 0.03, len(u)))
    return g[rng.permutation(len(g))]


def by_raster_rows(oracle, cloud, view=GRID_VIEW):
    """The same Gaussians ordered by the raster row, then the column, that the view sees them at: chunks of 64 neighbours."""
    sc = view_of(oracle, cloud, view)
    oc = sc.g["mu"][:, :3].astype(np.float64) - sc.origin.astype(np.float64)       # the unrotated camera looks along +z
    col, row = oc[:, 0] / oc[:, 2], oc[:, 1] / oc[:, 2]
    return np.ascontiguousarray(cloud.g[np.lexsort((col, np.floor(row * sc.h / 16.0)))])       # bands of 8 pixel rows, left to right


P136, CUBE, T96, NOREF, MANY = (136, 136, 2, 2, 0.0), (200, 136, 5, 5, 0.0), (96, 64, 4, 3, 0.0), (100, 100, 16, 16, 0.0), (256, 256, 4, 4, 0.0)
CLOUDS = {
    "grid": (_grid_cloud, GRID_FRAMES),
    "grid-thresholds": (_grid_cloud, THRESHOLD_FRAMES),
    "grid-cameras": (_grid_cloud, CAMERA_FRAMES),
    # family 2: tiles that are no multiple of 32, 8 or 4 pixels; a truncated tile size; grids and tiles that are not square
    "p136": (lambda o: _uniform_cloud(o, 31, 300, 0.01, 0.05), [frame(P136)]),
    "cube": (lambda o: _uniform_cloud(o, 32, 400, 0.01, 0.05, (0.02, 0.98, 0.02, 0.7)), [frame(CUBE)]),
    "t96": (lambda o: _uniform_cloud(o, 33, 200, 0.01, 0.05, (0.02, 0.8, 0.02, 0.98)), [frame(T96)]),
    "narrow": (_narrow_cloud, [frame(NARROW_FUSED), frame(NARROW_PAIR), frame(NARROW_ONE)]),
    # family 6: tile_w = 6, row stride 96 != 100 -- no refine, with device binning (fused) and with host lists (the cell kernel alone)
    "norefine": (lambda o: _uniform_cloud(o, 36, 300, 0.02, 0.1), [frame(NOREF), frame(NOREF, mode="lists")]),
    # family 7: N > 4096 -- eps_eff scales with 4096 / N; the chunk test is still off by default
    "many": (lambda o: _uniform_cloud(o, 37, 6000, 0.015, 0.05), [frame(MANY)]),
}
_clouds = {}


def cloud(oracle, name):
    """Settled once per process.  "grid-rows": the settled grid cloud in raster-row order (family 8)."""
    if name not in _clouds:
        if name == "grid-rows":
            base = cloud(oracle, "grid")
            _clouds[name] = Scene(name=name, g=by_raster_rows(oracle, base), views={}, drawn=base.drawn, removed=base.removed,
                                  frames=[frame(GRID_VIEW, chunks=True), frame(GRID_VIEW)])
        else:
            build, frames = CLOUDS[name]
            _clouds[name] = settle(oracle, name, build(oracle), frames)
    return _clouds[name]


ALL_CLOUDS = list(CLOUDS) + ["grid-rows"]
# (cloud, frame) of every frame the GPU suite renders
CASES = [(name, fr) for name in CLOUDS if name != "grid-cameras" for fr in CLOUDS[name][1] if not fr.chunks]
CASE_IDS = [f"{name}-{fr.name}" for name, fr in CASES]


# ---- the oracle's pixels ----
def lit_sample(oracle, cloud, fr, p, seed=5, most=128, work=2e8):
    """A seeded sample of pixels of lit cells and the oracle's radiance there: at most `most`, fewer where the tiles' lists are long (the
    oracle's cost per pixel is 5 n^2 terms).  (pixels, radiance float64, peak)"""
    key = ("_sample", fr.name)
    if key not in cloud:
        sc = view_of(oracle, cloud, fr.view)
        rng = np.random.default_rng(seed)
        lists = frame_lists(oracle, cloud, fr)
        if fr.mode == "none":
            tiles, longest = None, sc.n
        elif lists is None:
            tiles, longest = sc.ref, max(map(len, tile_lists(sc.ref)))
        else:
            off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
            tiles = dict(sc.ref, offsets=off, indices=np.concatenate(lists).astype(np.uint32))
            longest = max(map(len, lists))
        k = int(min(most, max(4, work / (5.0 * max(longest, 1) ** 2))))
        pool = np.concatenate([cell_pixels(p.L, key_) for key_ in sorted(p.cells_lit)])
        pix = np.sort(rng.choice(pool, min(k, len(pool)), replace=False)).astype(np.uint32)
        kinds = {"vcl": oracle.EXP_VCL, "libm": oracle.EXP_LIBM}
        _, rad = oracle.render(sc.w, sc.h, sc.plane, sc.origin, sc.g, tiles, exp_kind=kinds[fr.exp], pixels=pix, threads=8, want_image=False)
        cloud[key] = (pix, rad.astype(np.float64), float(max(1.0, np.abs(rad).max())))
    return cloud[key]
