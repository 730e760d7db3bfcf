"""Scenes that sit on the kernels' fixed capacities, one element either side (tests/test_gpu_boundaries.py renders them on
the GPU, tests/test_boundary_scenes.py checks on the CPU that they can see what they are meant to see).

A capacity bug (`<` for `<=`, a slot written at pos == CAP, a last element left out of a hand-over, a count saturated at the limit)
loses or doubles ONE Gaussian of a list of `cap - 1`, `cap` or `cap + 1`.  In a cloud of a thousand faint Gaussians one of them
moves a pixel by less than the parity tolerance, so the Gaussians at the indices where such a bug bites are MARKERS: strong, on the
view axis, each with a colour of its own.  `marker_effects` measures, with the oracle alone, what leaving each marker out does to
the checked pixels; the CPU suite holds that against ten times the tolerance the GPU test applies.

The capacities (csrc/vrt_kernels.h, vrt_block_kernel.hip, vrt_hip_api.cpp, vrt_hip_ctx.hpp):
  PRUNE_PL 16 | PL 24 | light_cells 24 | dense_threshold = PCAP 96 | chunk size 64 | TCAP 1024 | DCAP 1024 | TableCfg::TC 2048 |
  cstride min(n, 4096) | chunk test by default beyond 8192 | MAX_FUSED_CELLS 64
"""
import numpy as np

TOL = 1e-4          # parity tolerance of the GPU suite (tests/test_gpu_parity.py), times max(1, peak) on the dense and table paths
TOL_NOCULL = 2e-5   # the full sum in another association: where the block kernel shades the block
MARKER_FACTOR = 10  # a marker moves a checked pixel by at least this many tolerances

PRUNE_PL, PL, LIGHT_CELLS, PCAP, CHUNK, TCAP, DCAP, TABLE_TC, CSTRIDE_MAX, CHUNKS_DEFAULT_N, MAX_FUSED_CELLS = 16, 24, 24, 96, 64, 1024, 1024, 2048, 4096, 8192, 64
SQRT_2PI = 2.5066282746


def marker_indices(cap, n, chunked=False):
    """Where an off-by-one at `cap` would bite in a list of n: the first, the last, the slot before the limit and the one at it;
    with the chunk test also both sides of the first chunk border and the first and last member of the last chunk."""
    idx = {0, cap - 1, cap, n - 1}
    if chunked:
        idx |= {CHUNK - 1, CHUNK, ((n - 1) // CHUNK) * CHUNK, n - 1}
    return sorted(i for i in idx if 0 <= i < n)


def tolerance(n, peak):
    """The GPU tests' tolerance for an all-visible cloud of n with every cull off: the block kernel shades lists up to PL (the same
    sum as the reference's, re-associated), the dense and table kernels everything longer."""
    return TOL_NOCULL if n <= PL else TOL * max(1.0, float(peak))


class Scene(dict):
    __getattr__ = dict.__getitem__


def _camera(oracle, w, h):
    cam, _ = oracle.cli_camera(w, h)
    return oracle.camera_plane(cam), oracle.camera_view(cam), np.array(cam.position[:], np.float32)


def _brightest(rad, k):
    lum = np.asarray(rad, np.float64)[:, :3].sum(1)
    return np.sort(np.argsort(-lum, kind="stable")[:k]).astype(np.uint32)


def cloud(oracle, cap, n, w=16, h=16, chunked=False, compact=False, npix=3, seed=None, threads=8):
    """n Gaussians around the view axis of which every ray of the w x h image (one tile) sees all with cull_eps = 0 -- the CLI
    camera's image spans +-45 degrees, so on 16x16 pixels they are WIDE (sigma ~ 1: at the image corner d^2 / 2 sigma^2 stays far
    below the ~87 where Exp gives 0) -- and faint (the whole cloud has optical depth ~1 whatever n).  compact: narrow ones instead
    (sigma 0.012 .. 0.018 within 0.05 of the axis: Exp gives 0 beyond 13 sigma, 6 pixels of a 256-pixel image, so that the circular
    cone of a cell 16 pixels away keeps none), for large images where only the cells that meet at the centre are to hold them --
    and those hold them all.
    The markers sit ON the axis at depths of their own.  Checked pixels: brightest first in the oracle's image -- of the whole scene
    while that is affordable (n <= 200), of the markers alone beyond (the cloud is nearly flat across the pixels that see them)."""
    rng = np.random.default_rng(1000 * cap + n if seed is None else seed)
    plane, view, origin = _camera(oracle, w, h)
    s_lo, s_hi, spread, s_mark = (0.012, 0.018, 0.02, 0.018) if compact else (0.9, 1.3, 0.15, 0.5)
    off = rng.normal(size=(n, 3))
    mu = (np.clip(off, -2.5, 2.5) if compact else off) * spread + np.array([0, 0, 1.0])
    sigma = rng.uniform(s_lo, s_hi, n)
    mag = rng.uniform(0.4, 1.6, n) / (n * SQRT_2PI * sigma)        # optical depth of the cloud ~ 1
    alb = rng.uniform(0.1, 1.0, size=(n, 4))
    markers = marker_indices(cap, n, chunked)
    for j, k in enumerate(markers):
        mu[k] = (0.0, 0.0, 0.55 + 0.9 * (j + 0.5) / len(markers))
        sigma[k] = s_mark
        mag[k] = 0.25 / (SQRT_2PI * s_mark)
        alb[k] = [(1.0, 0.3, 0.2, 1.0), (0.2, 1.0, 0.3, 1.0), (0.3, 0.2, 1.0, 1.0), (1.0, 1.0, 0.2, 1.0)][j % 4]
    g = oracle.gaussians(alb, mu, sigma, mag)
    tiles = oracle.tile_gaussians(2.0, 2.0, g, view)
    assert tiles["w"] == tiles["h"] == 1 and tiles["offsets"][1] == n     # one tile that holds the whole scene
    if n <= 200:
        _, img = oracle.render(w, h, plane, origin, g, tiles, want_image=False, threads=threads)
    else:
        gm = g[markers]
        _, img = oracle.render(w, h, plane, origin, gm, oracle.tile_gaussians(2.0, 2.0, gm, view), want_image=False, threads=threads)
    return Scene(g=g, n=n, cap=cap, w=w, h=h, tw=2.0, th=2.0, plane=plane, view=view, origin=origin, tiles=tiles, markers=markers,
                 pixels=_brightest(img, npix))


def all_rays_see_all(sc):
    """With cull_eps = 0 a ray keeps a Gaussian unless Exp(-d^2 / 2 sigma^2) is exactly 0 (argument beyond ~87): true for
    every ray of the image and every Gaussian of the scene?  (float64 restatement, with a wide margin: 60.)"""
    xs, ys, zs = (np.asarray(a, np.float64) for a in sc.plane)
    d = np.stack([xs, ys, zs], 1) - sc.origin.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    oc = sc.g["mu"][:, :3].astype(np.float64) - sc.origin.astype(np.float64)
    t = d @ oc.T
    perp2 = (oc * oc).sum(1)[None, :] - t * t
    return bool((perp2 / (2.0 * sc.g["sigma"].astype(np.float64) ** 2)[None, :] < 60.0).all())


def render_oracle(oracle, sc, g=None, pixels=None, threads=8):
    g = sc.g if g is None else g
    tiles = sc.tiles if g is sc.g else oracle.tile_gaussians(sc.tw, sc.th, g, sc.view)
    return oracle.render(sc.w, sc.h, sc.plane, sc.origin, g, tiles, pixels=sc.pixels if pixels is None else pixels, threads=threads)


def marker_effects(oracle, sc, threads=8):
    """{marker index: largest change of a checked pixel's radiance when that Gaussian is left out}, and the peak of the full
    scene on the checked pixels.  The oracle alone."""
    _, full = render_oracle(oracle, sc, threads=threads)
    out = {}
    for k in sc.markers:
        _, rad = render_oracle(oracle, sc, g=np.delete(sc.g, k), threads=threads)
        out[k] = float(np.abs(rad.astype(np.float64) - full).max())
    return out, float(full.max())


# ---- one 32x32-pixel cell whose list holds n narrow Gaussians of which no ray sees more than a few ----
def lattice(oracle, cap, n, threads=8):
    """32 x 32 pixels = one tile = one cell; n narrow Gaussians on a 10 x 10 lattice over the image (spacing 0.9 at the depth of
    the scene, 2.9 pixels), sigma 0.12: at the default cull a ray keeps what lies within ~6 sigma = 0.7 of it, a handful.  The
    cell's list holds all n, so its length -- not a ray's or a block's -- is what crosses `cap` (dense_threshold 96, light_cells
    24).  Markers (magnitude 4 against 1) at 0, cap - 1, cap, n - 1; every pixel is checked."""
    w = h = 32
    plane, view, origin = _camera(oracle, w, h)
    rng = np.random.default_rng(7000 + n)
    k = np.arange(n)
    # lattice sites in an order that spreads consecutive indices over the image (37 is coprime to 100)
    site = (k * 37) % 100
    mu = np.stack([(site % 10 - 4.5) * 0.9, (site // 10 - 4.5) * 0.9, np.ones(n)], 1) + rng.normal(size=(n, 3)) * 0.02
    sigma = np.full(n, 0.12)
    mag = rng.uniform(0.8, 1.2, n)
    alb = rng.uniform(0.2, 1.0, size=(n, 4))
    markers = marker_indices(cap, n)
    for j in markers:
        mag[j] = 4.0
        alb[j] = (1.0, 1.0, 1.0, 1.0)
    g = oracle.gaussians(alb, mu, sigma, mag)
    tiles = oracle.tile_gaussians(2.0, 2.0, g, view)
    assert tiles["offsets"][1] == n
    return Scene(g=g, n=n, cap=cap, w=w, h=h, tw=2.0, th=2.0, plane=plane, view=view, origin=origin, tiles=tiles, markers=markers,
                 pixels=np.arange(w * h, dtype=np.uint32))


def visible_per_ray(sc, cull_eps=1e-9):
    """How many Gaussians each ray keeps at most: sigma * mag * exp(-x) >= cull_eps (the level-wise thresholds of the kernels are
    higher, so they keep no more than this).  [h * w] counts."""
    xs, ys, zs = (np.asarray(a, np.float64) for a in sc.plane)
    d = np.stack([xs, ys, zs], 1) - sc.origin.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    oc = sc.g["mu"][:, :3].astype(np.float64) - sc.origin.astype(np.float64)
    t = d @ oc.T
    x = ((oc * oc).sum(1)[None, :] - t * t) / (2.0 * sc.g["sigma"].astype(np.float64) ** 2)[None, :]
    q = np.abs(sc.g["sigma"].astype(np.float64) * sc.g["magnitude"])
    return (q[None, :] * np.exp(-x) >= cull_eps).sum(1)


# ---- `fast = __ballot(nl > PL) == 0`: one lane over the limit sends the whole block to the dense path ----
def one_lane_over(oracle, threads=8):
    """16 x 16 pixels (four blocks, one tile): 24 wide Gaussians that every ray keeps at the default cull, plus a narrow one
    (index 24, the last of the list) on the ray of pixel (4, 4) of block 0, which its neighbours' rays (0.6 apart at that depth)
    drop: one lane of one block holds 25, every other lane 24."""
    w = h = 16
    plane, view, origin = _camera(oracle, w, h)
    rng = np.random.default_rng(2425)
    n = PL + 1
    mu = rng.normal(size=(n, 3)) * 0.15 + np.array([0, 0, 1.0])
    sigma = rng.uniform(1.3, 1.6, n)
    mag = rng.uniform(0.02, 0.05, n)
    alb = rng.uniform(0.1, 1.0, size=(n, 4))
    px = 4 * w + 4
    o = origin.astype(np.float64)
    d = np.array([plane[0][px], plane[1][px], plane[2][px]], np.float64) - o
    mu[PL] = o + d * (5.0 / d[2])                       # on that pixel's ray, at the depth of the cloud
    sigma[PL], mag[PL], alb[PL] = 0.04, 2.0, (1.0, 1.0, 1.0, 1.0)
    g = oracle.gaussians(alb, mu, sigma, mag)
    tiles = oracle.tile_gaussians(2.0, 2.0, g, view)
    assert tiles["offsets"][1] == n
    return Scene(g=g, n=n, cap=PL, w=w, h=h, tw=2.0, th=2.0, plane=plane, view=view, origin=origin, tiles=tiles, markers=[PL],
                 pixels=np.arange(w * h, dtype=np.uint32), lane_pixel=px)


# ---- PRUNE_PL: lists up to 16 long are pruned, longer ones are not ----
def prunable(oracle, n, faint=3):
    """16 x 16 pixels: n wide Gaussians that every ray keeps at the default cull.  The last `faint` of them carry
    sigma * mag * exp(-x) between 5e-7 and 1e-6 on every ray (sigma 4): above the ray level's threshold (1e-9 * 1365 / n < 1e-7)
    and, summed, below the prune's budget (6 * 1365 * 1e-9 = 8.2e-6) -- the prune drops all of them from every list it looks at."""
    w = h = 16
    plane, view, origin = _camera(oracle, w, h)
    rng = np.random.default_rng(1600 + n)
    mu = rng.normal(size=(n, 3)) * 0.15 + np.array([0, 0, 1.0])
    sigma = rng.uniform(1.3, 1.6, n)
    mag = rng.uniform(0.03, 0.08, n)
    alb = rng.uniform(0.1, 1.0, size=(n, 4))
    sigma[n - faint:] = 4.0
    mag[n - faint:] = 1e-6 / 4.0
    g = oracle.gaussians(alb, mu, sigma, mag)
    tiles = oracle.tile_gaussians(2.0, 2.0, g, view)
    assert tiles["offsets"][1] == n
    return Scene(g=g, n=n, cap=PRUNE_PL, w=w, h=h, tw=2.0, th=2.0, plane=plane, view=view, origin=origin, tiles=tiles, markers=[],
                 pixels=np.arange(w * h, dtype=np.uint32), faint=faint)


# the all-visible clouds the GPU tests render with every cull off: (name of the limit, cap, image, chunk test, compact)
CLOUD_LIMITS = [("PL", PL, 16, 16, False, False), ("DCAP/TCAP", DCAP, 16, 16, False, False), ("TableCfg::TC", TABLE_TC, 16, 16, False, False)]
CLOUD_CASES = [(name, cap, n, w, h, chunked, compact) for (name, cap, w, h, chunked, compact) in CLOUD_LIMITS for n in (cap - 1, cap, cap + 1)]
# cstride: a tile of 72 cells (256 x 288 pixels), the cloud confined to the cells at its centre
CSTRIDE_CASES = [("cstride", CSTRIDE_MAX, n, 256, 288, False, True) for n in (CSTRIDE_MAX - 1, CSTRIDE_MAX, CSTRIDE_MAX + 1)]
# the chunk test (VRT_HIP_CHUNKS=2): full and ragged last chunks
CHUNK_CASES = [("chunk", CHUNK * ((n + 1) // CHUNK), n, 16, 16, True, False) for n in (63, 64, 65, 127, 128, 129)]
LATTICE_CASES = [(cap, n) for cap in (LIGHT_CELLS, PCAP) for n in (cap - 1, cap, cap + 1)]
