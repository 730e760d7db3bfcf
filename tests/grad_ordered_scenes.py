"""Model, record sets and bundles for the ordered gradient tables (vrt_hip_set_grad_ordered, csrc/vrt_grad_ordered_kernel.hip):
tests/test_gpu_grad_ordered.py holds the GPU's table to `ordered_reduce` of the GPU's own records BIT FOR BIT,
tests/test_grad_ordered_scenes.py checks on the CPU that the model is the order include/vrt_hip.h states, that it is a sum, and that the
record sets can tell that order from four others.

The order (normative; include/vrt_hip.h, "ordered gradient tables").  The records reach the reduction in CONSUMED ORDER: by Gaussian,
then ray id, then the record's place in its ray.  For Gaussian j with records rho_0 .. rho_{m-1} in that order and each column c:
    lane l = 0..63 holds a_l = (((+0 + rho_l[c]) + rho_{l+64}[c]) + rho_{l+128}[c]) + ...            (+0 where there is no record)
    six steps s = 1, 2, 4, 8, 16, 32 in this order: a_l <- a_l + a_{l xor s}, every lane from the values before the step
    table[j, c] <- table[j, c] + a_0
in float32, every add rounded on its own.  Rows of Gaussians without records and columns outside `cols` are not written.

Depth.  A segment of m records is summed ceil(m / 64) + 6 adds deep (`depth`), the add into the table not counted: against the exact sum
the result is within depth * 2^-24 * sum |addend| to first order (`sum_bound` adds the second-order term).
"""
import functools

import numpy as np

import grad_bundle_scenes as G
from grad_bundle_scenes import RAY_LCAP, RAY_PL  # noqa: F401

NREC = 9                     # floats per record: the table's columns 0..8
STRIDE = 12                  # floats per row of the table
RADIANCE_COLS = tuple(range(0, 9))
TRANS_COLS = tuple(range(4, 9))
WRONG = ("sequential", "steps_down", "stride32", "from_table")
SEGMENTS = (1, 63, 64, 65, 128, 129, 4096)
K_RAYS = (1, 63, 64, 65, 129)
CAMERA = np.array([0.0, 0.0, -4.0], np.float32)      # the CLI camera's position


def depth(m):
    return -(-int(m) // 64) + 6


def sum_bound(m, sum_abs):
    """|ordered float32 sum - exact sum| of m addends whose absolute values sum to sum_abs"""
    u = 2.0 ** -24
    return ((1.0 + u) ** depth(m) - 1.0) * sum_abs


def segments(gauss):
    """(j, lo, hi) of every run of equal keys in consumed order"""
    gauss = np.asarray(gauss)
    if not len(gauss):
        return []
    cut = np.concatenate([[0], np.nonzero(gauss[1:] != gauss[:-1])[0] + 1, [len(gauss)]])
    return [(int(gauss[lo]), int(lo), int(hi)) for lo, hi in zip(cut[:-1], cut[1:])]


def _lanes(seg, width, start=None):
    """a_l of the first stage: [width, cols] float32, lane l over records l, l + width, ...; start: lane 0 begins there instead of at +0"""
    m = len(seg)
    rounds = -(-m // width)
    pad = np.zeros((rounds * width, seg.shape[1]), np.float32)       # +0 where there is no record: x + (+0) = x for every x the sum can hold
    pad[:m] = seg
    a = np.zeros((width, seg.shape[1]), np.float32)
    if start is not None:
        a[0] = start
    for k in range(rounds):
        a = a + pad[k * width:(k + 1) * width]
    return a


def _butterfly(a, steps):
    lanes = np.arange(len(a))
    for s in steps:
        a = a + a[lanes ^ s]
    return a


def ordered_reduce(gauss, rows, table0, cols=RADIANCE_COLS, variant=None):
    """The table [N, 12] float32 after the reduction of the records (gauss [m] in consumed order, rows [m, 9]) into table0.  Works on the
    bits: cells outside the written ones keep whatever table0 held (NaN payloads, -0).  variant: one of WRONG, another order."""
    table = np.array(table0, np.float32, copy=True)
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, NREC)
    cols = list(cols)
    assert all(a <= b for a, b in zip(gauss[:-1], gauss[1:])), "records are not in consumed order"
    with np.errstate(all="ignore"):
        for j, lo, hi in segments(gauss):
            seg = rows[lo:hi][:, cols]
            old = table[j, cols].copy()
            if variant == "sequential":
                a0 = np.zeros(len(cols), np.float32)
                for rec in seg:
                    a0 = a0 + rec
                new = old + a0
            elif variant == "steps_down":
                new = old + _butterfly(_lanes(seg, 64), (32, 16, 8, 4, 2, 1))[0]
            elif variant == "stride32":
                new = old + _butterfly(_lanes(seg, 32), (1, 2, 4, 8, 16))[0]
            elif variant == "from_table":
                new = _butterfly(_lanes(seg, 64, start=old), (1, 2, 4, 8, 16, 32))[0]      # lane 0 starts from the table's value, not +0
            else:
                assert variant is None, variant
                new = old + _butterfly(_lanes(seg, 64), (1, 2, 4, 8, 16, 32))[0]
            table[j, cols] = new
    return table


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- crafted record sets ----
def crafted(seed=1):
    """(gauss [m], rows [m, 9], N): one segment of each length of SEGMENTS, on Gaussians with gaps between them, mixed magnitudes (eight
    decades) and signs, a few exact zeros and a run that cancels."""
    rng = np.random.default_rng(9000 + seed)
    keys = np.cumsum(rng.integers(1, 4, len(SEGMENTS)))             # gaps: Gaussians without records in between
    gauss = np.repeat(keys, SEGMENTS).astype(np.uint32)
    m = len(gauss)
    rows = (rng.uniform(-1.0, 1.0, size=(m, NREC)) * 10.0 ** rng.uniform(-4, 4, size=(m, NREC))).astype(np.float32)
    rows[rng.random(size=(m, NREC)) < 0.02] = 0.0
    rows[5:m:97, 3] = -0.0
    half = slice(m - 4096, m - 4096 + 1000)
    rows[m - 3096:m - 2096] = -rows[half]                            # a run of the longest segment cancels an earlier one
    return gauss, rows, int(keys[-1]) + 2


def random_table(n, seed=3):
    """A table [n, 12] of random values: what a reduction adds to"""
    return np.random.default_rng(seed).uniform(-2.0, 2.0, size=(n, STRIDE)).astype(np.float32)


def poison(table, written):
    """table with -0.0 and NaNs of distinct payloads in every cell where `written` [n, 12] is False"""
    t = bits(table).copy()
    idx = np.nonzero(~written)
    pat = np.where((idx[0] + idx[1]) % 3 == 0, 0x80000000, 0x7FC00000 + ((idx[0] * STRIDE + idx[1]) & 0xFFFFF) + 1).astype(np.uint32)
    t[idx] = pat
    return t.view(np.float32)


def written_cells(n, gauss, cols):
    w = np.zeros((n, STRIDE), bool)
    if len(gauss):
        w[np.ix_(np.unique(gauss), list(cols))] = True
    return w


# ---- bundles ----
def k_rays(oracle, k):
    """k rays through one Gaussian (index 1; two more that no ray keeps either side of it): every ray keeps exactly that one, so its
    segment has exactly k records"""
    rng = np.random.default_rng(8100 + k)
    mu = np.array([[3.0, 3.0, 1.0], [0.0, 0.0, 1.0], [-3.0, -3.0, 1.0]])
    g = oracle.gaussians(rng.uniform(0.1, 1.0, size=(3, 4)), mu, np.array([0.05, 0.3, 0.05]), np.array([1.0, 0.9, 1.0]))
    target = mu[1][None, :] + rng.normal(size=(k, 3)) * [0.15, 0.15, 0.0]
    d = G.normalise(target - G.ORIGIN.astype(np.float64))
    assert not G.undecided(G.ORIGIN, d, g).any()
    sc = G.GradScene(f"rays {k}", g, G.ORIGIN, d, G.seeded_gr(k, 700 + k), [1])
    assert all(list(l) == [1] for l in sc.lists())
    return sc


AIMED_WINDOW = 0.01   # tools/ray_bundles.py zooms onto 0.03 x 0.03 of `-g 64`; on `-g 16` that window leaves 16 of the 256 Gaussians within
                      # float32's margin of some ray's cull decision, above `settled`'s cap of 5 %; this one leaves 10, and its rays keep 6 or 7


def aimed_rays(g, window=AIMED_WINDOW):
    """The 64 x 64 pinhole of the CLI camera zoomed onto window x window of the grid around one Gaussian (tools/ray_bundles.py's zoom bundle)"""
    centre = g["mu"][len(g) // 2 + int(round(len(g) ** 0.5)) // 2, :3].astype(np.float64)
    u = (np.arange(64) - 31.5) / 64 * window
    target = centre[None, :] + np.stack([np.tile(u, 64), np.repeat(u, 64), np.zeros(4096)], 1)
    return CAMERA, G.normalise(target - CAMERA.astype(np.float64))


def aimed(oracle):
    """The aimed bundle on `-g 16`, without the Gaussians whose cull float32 could decide either way (at most 5 % may go: `settled`)"""
    g0 = oracle.grid_scene(16)
    o, d = aimed_rays(g0)
    g = G.settled(g0, o, d)
    hits = G.R.kept(o, d, g).sum(0)
    return G.GradScene("aimed 64x64", g, o, d, G.seeded_gr(len(d), 710), list(np.argsort(-hits, kind="stable")[:4]))


@functools.lru_cache(maxsize=None)
def _bundles(oracle):
    return {sc.name: sc for sc in [k_rays(oracle, k) for k in K_RAYS] + [aimed(oracle)]}


def bundle(oracle, name):
    """A bundle of this file by name, or a scene of grad_bundle_scenes"""
    b = _bundles(oracle)
    return b[name] if name in b else G.scene(oracle, name)


def record_count(lens, two):
    """Records of a bundle whose rays keep `lens` Gaussians: one per kept Gaussian, `two` (the radiance gradient) two for a ray that keeps
    more than RAY_PL"""
    lens = np.asarray(lens, np.int64)
    return int(np.where(lens > RAY_PL, (2 if two else 1) * lens, lens).sum())
