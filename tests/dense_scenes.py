"""Scenes for the exact dense body (csrc/vrt_dense_block.hpp: dense_shade_block, the arithmetic of the exact dense kernel and of the
table kernel's fallback) and a float64 model of the decisions it takes per 8x8 block: the depth order, the deal of the emitters in
chunks of six, and which (chunk, absorber) visits the saturation tests settle without the term-by-term loop.
tests/test_gpu_dense.py renders them on the GPU, tests/test_dense_scenes.py checks on the CPU that they can see what they are meant
to see.  numpy and the oracle only: no GPU, no product import.

The body sorts a block's candidates by depth along the block's axis (rank sort, ties broken by list position), deals chunks of
EC = 6 consecutive ranks to wave w, w + DW, ... (the last chunk padded with its first member) and lets every wave stream ALL
candidates as absorbers for its chunk.  With r_j = 1 / (sqrt2 sigma_j), m_j = mubar_j r_j and, per ray, the chunk's sample range
[s_min, s_max] = [min_e (mubar_e - 4 sigma_e), max_e mubar_e]:
    zero    m_j >= SAT and (s_max - mubar_j) r_j <= -SAT_M on all 64 rays: every term is exactly 0, the absorber is skipped
    common  m_j >= SAT and (s_min - mubar_j) r_j >=  SAT_M on all 64 rays: every term is exactly -2 A_j, one fma
    full    everything else: 5 EC Erf terms
SAT is where the Erf variant is exactly +-1 in fp32 (erf_saturation<>), SAT_M = SAT + 1e-3.  One visit = one absorber seen by
one chunk: a block of cnt candidates makes ceil(cnt / 6) cnt of them, whatever DW.
"""
import numpy as np

from boundary_scenes import MARKER_FACTOR, PL, Scene, marker_effects, render_oracle, tolerance  # noqa: F401 (re-exported)

EXP_LIBM, EXP_VCL, EXP_FAST, EXP_SPLINE = 0, 1, 2, 3          # oracle/oracle.py and include/vrt_hip.h use the same numbers
ERF_LIBM, ERF_AS, ERF_SPLINE, ERF_SPLINE_MIRROR, ERF_TAYLOR = 0, 1, 2, 3, 4
SAT = {ERF_LIBM: 4.2, ERF_AS: 5.5, ERF_SPLINE: 3.1, ERF_SPLINE_MIRROR: 2.9, ERF_TAYLOR: 2.0}      # erf_saturation<>, vrt_device_math.h
ERF_NAMES = {ERF_LIBM: "libm", ERF_AS: "as", ERF_SPLINE: "spline", ERF_SPLINE_MIRROR: "mirror", ERF_TAYLOR: "taylor"}
EXP_NAMES = {EXP_LIBM: "libm", EXP_VCL: "vcl", EXP_FAST: "fast", EXP_SPLINE: "spline"}
# the pairs of VRT_DISPATCH_EXP_ERF (vrt_kernels_common.hpp)
PAIRS = ((EXP_LIBM, ERF_LIBM), (EXP_LIBM, ERF_AS), (EXP_VCL, ERF_LIBM), (EXP_VCL, ERF_AS), (EXP_FAST, ERF_AS), (EXP_SPLINE, ERF_AS),
         (EXP_VCL, ERF_SPLINE), (EXP_VCL, ERF_SPLINE_MIRROR), (EXP_VCL, ERF_TAYLOR))
ERF_JUMP = {ERF_SPLINE_MIRROR: 0.107, ERF_TAYLOR: 4.7e-3}     # spline_erf_mirror at 0, taylor_erf at +-2 (tests/test_gpu_parity.py)
EC = 6
WAVES = (4, 8, 16)               # VRT_HIP_DENSE_WAVES; 17 = 16 waves without the saturation tests
SHAPES = (4, 8, 16, 17)
MARGIN = 2e-3                    # the model's thresholds are evaluated at (1 +- MARGIN); the kernel's re-association noise is ~1e-6
# every residue mod 6 with five chunks (and the hand-over from the block kernel: cells up to 96); the second round of 8 and of 16
# waves (97: the first cell of the dense queue); the second round of 16 waves' second chunk
LENGTHS = (25, 26, 27, 28, 29, 30, 48, 49, 96, 97, 192, 193)
PAIR_LENGTHS = (97, 30)
TIE_GROUPS = (2, 3, 7)           # seven copies cannot fit into one chunk
RAGGED = {"one-tile-20x12": (20, 12, 2.0, 2.0), "four-tiles-20x20": (20, 20, 1.0, 1.0)}
SQRT_2PI = 2.5066282746310002
COLOURS = [(1.0, 0.3, 0.2, 1.0), (0.2, 1.0, 0.3, 1.0), (0.3, 0.2, 1.0, 1.0), (1.0, 1.0, 0.2, 1.0)]


def deal_ranks(n):
    """The ranks, in depth order, where the deal can lose or double an emitter: the first, the members of the last chunk (the
    padding repeats its first), and both sides of the end of the first round of 4, 8 and 16 waves."""
    idx = {0} | set(range(n - (n % EC or EC), n))
    for dw in WAVES:
        idx |= {EC * dw - 1, EC * dw}
    return sorted(i for i in idx if 0 <= i < n)


# ---- what the kernel sees, in float64 ----
def blocks_of(sc):
    """The 8x8 blocks that hold a pixel, as the kernels walk them (tile, 32x32 cell, block): per block the 64 lanes' pixel indices --
    a lane beyond the tile's edge shades the clamped pixel and writes nothing -- and which lanes write."""
    tile_w, tile_h = int(np.float32(sc.w) * np.float32(sc.tw) / np.float32(2)), int(np.float32(sc.h) * np.float32(sc.th) / np.float32(2))
    out = []
    for ty in range(sc.tiles["h"]):
        for tx in range(sc.tiles["w"]):
            for by in range(-(-tile_h // 8)):
                for bx in range(-(-tile_w // 8)):
                    pxt, pyt = bx * 8 + np.arange(64) % 8, by * 8 + np.arange(64) // 8
                    valid = (pxt < tile_w) & (pyt < tile_h)
                    pix = tx * tile_w + np.minimum(pxt, tile_w - 1) + sc.w * (ty * tile_h + np.minimum(pyt, tile_h - 1))
                    valid &= pix < sc.w * sc.h
                    out.append((np.minimum(pix, sc.w * sc.h - 1), valid))
    return out


def geometry(sc):
    if "_geom" in sc:
        return sc["_geom"]
    o32 = sc.origin.astype(np.float32)
    o = o32.astype(np.float64)
    d = np.stack([np.asarray(a, np.float64) for a in sc.plane], 1) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    oc = (sc.g["mu"][:, :3].astype(np.float32) - o32).astype(np.float64)        # gA: centre - origin, in fp32 (prep_frame_kernel)
    mubar = d @ oc.T                                                            # [ray, gaussian]
    d2 = np.maximum((oc * oc).sum(1)[None, :] - mubar * mubar, 0.0)
    s32 = sc.g["sigma"].astype(np.float32)
    r = (np.float32(1.0) / (np.float32(1.41421356237309504880) * s32)).astype(np.float64)   # gB.x, build_static_kernel
    sigma, mag = s32.astype(np.float64), sc.g["magnitude"].astype(np.float64)
    A = (sigma * mag / SQRT_2PI)[None, :] * np.exp(-d2 / (2.0 * sigma * sigma)[None, :])     # gB.z Exp(-d2 gB.y)
    sc["_geom"] = Scene(d=d, oc=oc, mubar=mubar, d2=d2, r=r, sigma=sigma, mag=mag, A=A)
    return sc["_geom"]


def keys(sc, lanes):
    """Depth of every Gaussian along the block's axis: the normalised sum of the rays of lanes 27, 28, 35 and 36."""
    G = geometry(sc)
    c = G.d[lanes[[27, 28, 35, 36]]].sum(0)
    return G.oc @ (c / np.linalg.norm(c))


def keys32(sc, lanes):
    """The same in float32, operation by operation as the kernel forms it (pixel_ray's normalisation, the sum of four, the
    reciprocal square root, the three products summed left to right).  A contraction into fma may move the last bit: equal rows give
    equal keys either way, which is all this is used for."""
    f = np.float32
    o = sc.origin.astype(f)
    p = np.stack([np.asarray(a, f) for a in sc.plane], 1)[lanes[[27, 28, 35, 36]]] - o
    nrm = np.sqrt(((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(f)).astype(f)
    d = (p / nrm[:, None]).astype(f)
    c = ((d[0] + d[1]).astype(f) + d[2]).astype(f) + d[3]
    c = (c * (f(1) / np.sqrt(((c[0] * c[0] + c[1] * c[1]).astype(f) + c[2] * c[2]).astype(f)))).astype(f)
    a = sc.g["mu"][:, :3].astype(f) - o
    return ((a[:, 0] * c[0] + a[:, 1] * c[1]).astype(f) + a[:, 2] * c[2]).astype(f)


def depth_order(sc, lanes=None):
    """The rank sort's result: list positions by ascending key, equal keys by ascending list position (`kk == ki && k < i`)."""
    return np.argsort(keys(sc, np.arange(64) if lanes is None else lanes), kind="stable")


def chunks(n):
    """The emitter chunks of a block of n candidates: per chunk the EC ranks its wave loads (the padding repeats the first)."""
    return [[i0 + e if i0 + e < n else i0 for e in range(EC)] for i0 in range(0, n, EC)]


def visit_total(counts):
    return sum(-(-c // EC) * c for c in counts)


def plan(sc, sat, margin=MARGIN):
    """The body's decisions for a scene of ONE block that keeps every Gaussian: the number of (chunk, absorber) visits and a
    (lower, upper) count of the `zero` and of the `common` ones, the thresholds m >= SAT, hi <= -SAT_M and lo >= SAT_M each taken at
    (1 + margin) for the lower and at (1 - margin) for the upper count."""
    assert sc.w == sc.h == 8
    G, n = geometry(sc), sc.n
    order = depth_order(sc)
    mub, sig, r = G.mubar[:64][:, order], G.sigma[order], G.r[order]
    m = mub * r
    sat_m = float(np.float32(sat) + np.float32(1e-3))
    zero, common = [0, 0], [0, 0]
    for ch in chunks(n):
        s_max = mub[:, ch].max(1)[:, None]
        s_min = (mub[:, ch] - 4.0 * sig[ch][None, :]).min(1)[:, None]
        hi, lo = (s_max - mub) * r, (s_min - mub) * r
        for k, scale in enumerate((1.0 + margin, 1.0 - margin)):
            front = m >= sat * scale
            zero[k] += int((front & (hi <= -sat_m * scale)).all(0).sum())
            common[k] += int((front & (lo >= sat_m * scale)).all(0).sum())
    total = visit_total([n])
    return Scene(total=total, zero=tuple(zero), common=tuple(common), full=(total - zero[1] - common[1], total - zero[0] - common[0]))


def absorption(sc):
    """Per ray S = sum_j 2 A_j: the largest exponent a sample of that ray can meet."""
    return 2.0 * geometry(sc).A.sum(1)


def skip_bound(sc, orad):
    """What skipping may change per pixel (16 waves against 17): the zero skip drops fma(A, 0, acc), exact; the common skip moves
    the -2 A_j of the skipped absorbers from each of a chunk's running sums into one of its own.  Both are sums of at most n terms of
    which none exceeds the total S, so each carries a rounding error below n 2^-24 S, one more rounding joins them, and 2 stands for
    the terms' own last bits: the exponent moves by at most (2n + 2) 2^-24 S, a sample's emission by 1.01 times that relative to
    itself (e^x - 1 <= 1.01 x here), and the samples of a pixel sum, with non-negative weights, to its radiance: L, its largest
    component.  4 2^-24 L for the Exp of an argument that moved and the products behind it."""
    L = np.asarray(orad, np.float64).max(1)
    return (2 * sc.n + 2) * 2.0 ** -24 * absorption(sc)[sc.pixels] * L * 1.01 + 4 * 2.0 ** -24 * L


def shape_bound(sc, orad):
    """What the number of waves may change per pixel: chunks are aligned multiples of six for every DW, so an emitter's `inner` is
    the same bits; the n non-negative terms of a ray are added in another order, within a wave and then across up to 16 waves."""
    return (sc.n + 16) * 2.0 ** -23 * np.asarray(orad, np.float64).max(1)


def seen(sc):
    """[ray, Gaussian]: the ray keeps the Gaussian with cull_eps = 0 (Exp's argument below 60, far from the ~87 where it gives 0)."""
    G = geometry(sc)
    return G.d2 / (2.0 * G.sigma ** 2)[None, :] < 60.0


def blocks_go_dense(sc):
    """Every block has a lane that keeps more than the block kernel's PL = 24 (one such lane sends the whole block to the dense
    path), and a lane that keeps every Gaussian of the scene: how many, over the blocks, keep them ALL (the dense body's candidates
    are what any of its rays keeps)."""
    s = seen(sc)
    assert all(s[pix].sum(1).max() > PL for pix, _ in blocks_of(sc))
    return sum(bool(s[pix].any(0).all()) for pix, _ in blocks_of(sc))


# ---- the scenes ----
def bare(oracle, alb, mu, sigma, mag, w=8, h=8, tw=2.0, th=2.0):
    """Gaussians under the narrow camera: 36 in front of the origin, the image plane 32 in front of the camera."""
    cam, _ = oracle.cli_camera(w, h, camera_offset=-36.0, focal=32.0)
    plane, view, origin = oracle.camera_plane(cam), oracle.camera_view(cam), np.array(cam.position[:], np.float32)
    g = oracle.gaussians(alb, mu, sigma, mag)
    return Scene(g=g, n=len(g), w=w, h=h, tw=tw, th=th, plane=plane, view=view, origin=origin, tiles=oracle.tile_gaussians(tw, th, g, view),
                 markers=[], pixels=np.arange(w * h, dtype=np.uint32))


def stack(oracle, n, seed=None, w=8, h=8, tw=2.0, th=2.0, groups=(), same_depth=False):
    """A depth stack on the view axis seen through a narrow angle (the image plane 32 in front of the camera, the stack 35 .. 66): as
    an 8x8 image one tile, one cell and ONE block, whose cell's other 15 blocks lie outside the tile.  Narrow Gaussians (sigma
    0.15 .. 0.4) in list order unrelated to depth, one in eight wide (1.2 .. 2): behind a chunk of narrow emitters most absorbers
    are saturated one way or the other, and a wide emitter in the chunk stretches its sample range to the front -- which a wrong
    s_min would not.  Optical depth of the stack ~1.5.
    groups: sizes of groups of exact copies of a centre (bit-equal keys; sigma, albedo and magnitude stay different);
    same_depth: every Gaussian at ONE centre.
    Markers (four times the magnitude, colours of their own) at deal_ranks(n) of the depth order and on one member of each group.
    Every pixel is checked."""
    rng = np.random.default_rng(31000 + n if seed is None else seed)
    mu = np.stack([rng.normal(0.0, 0.1, n), rng.normal(0.0, 0.1, n), rng.uniform(-1.0, 30.0, n)], 1)
    sigma = rng.uniform(0.15, 0.4, n)
    wide = rng.random(n) < 0.125
    sigma[wide] = rng.uniform(1.2, 2.0, int(wide.sum()))
    mag = 1.5 * rng.uniform(0.4, 1.6, n) / (n * SQRT_2PI * sigma)
    alb = rng.uniform(0.1, 1.0, size=(n, 4))
    members = []
    if same_depth:
        mu[:] = (0.02, -0.03, 14.0)
        members.append(np.arange(n))
    elif groups:
        free = rng.permutation(n)
        for size in groups:
            ids, free = np.sort(free[:size]), free[size:]
            mu[ids] = mu[ids[0]]
            members.append(ids)
    sc = bare(oracle, alb, mu, sigma, mag, w, h, tw, th)
    order = depth_order(sc, blocks_of(sc)[0][0])                   # magnitudes and colours do not move a key
    markers = {int(order[k]) for k in deal_ranks(n)}
    if not same_depth:
        markers |= {int(ids[len(ids) // 2]) for ids in members}
    for j, k in enumerate(sorted(markers)):
        mag[k] *= 4.0
        alb[k] = COLOURS[j % 4]
    sc["g"] = oracle.gaussians(alb, mu, sigma, mag)
    del sc["_geom"]                                                # (it holds the magnitudes)
    if sc.tiles["w"] == sc.tiles["h"] == 1:
        assert sc.tiles["offsets"][1] == n                         # the reference's tile test drops what lies closer than 1 behind the image plane
    sc.update(markers=sorted(markers), groups=members, order=order)
    return sc


def ties(oracle, same_depth=False):
    """The stack with bit-equal keys: groups of 2, 3 and 7 copies of a centre among 61, or 30 Gaussians at one centre."""
    return stack(oracle, 30, seed=31301, same_depth=True) if same_depth else stack(oracle, 61, seed=31300, groups=TIE_GROUPS)


def ragged(oracle, name):
    """A stack of 60 under a geometry whose blocks are cut: 20x12 pixels as one tile (blocks cut at the right and at the bottom), or
    20x20 pixels as 2x2 tiles of 10x10 (every tile's second block column and row hold two pixels)."""
    w, h, tw, th = RAGGED[name]
    return stack(oracle, 60, seed=31400 + w + h, w=w, h=h, tw=tw, th=th)


_scenes = {}


def scene(oracle, key):
    """('stack', n) | ('ties', same_depth) | ('ragged', name): built once per process, with the oracle's frame of the default pair."""
    if key not in _scenes:
        sc = {"stack": stack, "ties": ties, "ragged": ragged}[key[0]](oracle, key[1])
        sc["oimg"], sc["orad"] = render_oracle(oracle, sc)
        sc["orad"] = sc.orad.astype(np.float64)
        _scenes[key] = sc
    return _scenes[key]


def oracle_pair(oracle, sc, exp_kind, erf_kind, threads=8):
    """The oracle's radiance with another Exp / Erf pair."""
    key = ("_orad", exp_kind, erf_kind)
    if key not in sc:
        _, rad = oracle.render(sc.w, sc.h, sc.plane, sc.origin, sc.g, sc.tiles, exp_kind=exp_kind, erf_kind=erf_kind, pixels=sc.pixels,
                               want_image=False, threads=threads)
        sc[key] = rad.astype(np.float64)
    return sc[key]
