"""A numpy model of the ray plans (vrt_hip_ray_plan_create*, vrt_hip_set_ray_plan, csrc/vrt_ray_plan_kernel.hip) and the bundles that
tests/test_gpu_ray_plans.py runs planned and unplanned; tests/test_ray_plan_scenes.py checks on the CPU, with the oracle alone, that the
cases can tell the model from the ways a plan can go wrong and that the frozen-list pair is worth what the GPU suite holds it to.

A plan is the cull of a bundle run once and kept: per ray the list of kept scene indices in ascending order (ray_bundle_scenes.kept says
which), CSR at the caller's ray index; the rays whose list is longer than RAY_PL, which a planned call hands to the one-wave-per-ray
kernel; and what a planned call must report of itself -- the per-ray statistics of the unplanned call, and no test at all.
"""
import numpy as np

import grad_bundle_scenes as G
import ray_bundle_scenes as R
import ray_index_scenes as X
import ray_sort_scenes as RS
from ray_bundle_scenes import (RAY_LCAP, RAY_PL, coherent_rays, scattered_rays, stack, stack_rays, stack_with_side, wide_rays,  # noqa: F401
                               wide_stack)

WRONG = ("long_ge", "morton_order", "slot_order", "stale_queue", "offsets_shifted")
SIZES = (1, 63, 64, 65, 130)
MARKER_FACTOR = 10          # a marker ray's list difference is worth at least this many tolerances


class Plan:
    """offsets u64 [nrays + 1], entries u32, lens [nrays], queue: the ids of the long rays (a set: the device files them in any order)"""

    def __init__(self, offsets, entries, queue):
        self.offsets, self.entries, self.queue = np.asarray(offsets, np.uint64), np.asarray(entries, np.uint32), np.sort(np.asarray(queue, np.int64))
        self.lens = np.diff(self.offsets.astype(np.int64))

    def list_of(self, r):
        return self.entries[int(self.offsets[r]):int(self.offsets[r + 1])]

    def lists(self):
        return [self.list_of(r) for r in range(len(self.lens))]

    def info(self):
        """entries, short_rays, long_rays, longest, scratch_rays: vrt_hip_ray_plan_info's"""
        n = self.lens
        return {"rays": len(n), "entries": int(n.sum()), "short_rays": int((n <= RAY_PL).sum()), "long_rays": int((n > RAY_PL).sum()),
                "longest": int(n.max()) if len(n) else 0, "scratch_rays": int((n > RAY_LCAP).sum())}

    def stats(self):
        """vrt_hip_ray_stats of a planned call: a ray in the queue is shaded one wave per ray, every other lane = ray over its list"""
        long = np.zeros(len(self.lens), bool)
        long[self.queue[self.queue < len(long)]] = True
        short = self.lens[~long]
        return {"rays": len(self.lens), "short_rays": int((~long).sum()), "long_rays": int(long.sum()), "lane_entries": int(short.sum()),
                "lane_pairs": int((short.astype(np.int64) ** 2).sum()), "chunks_tested": 0, "chunks_kept": 0, "members_tested": 0,
                "scratch_rays": int((self.lens[long] > RAY_LCAP).sum())}

    def observed(self):
        """What a planned call sees of the plan, as one comparable value: every ray's list, the long rays, the statistics"""
        return ([tuple(l.tolist()) for l in self.lists()], tuple(self.queue.tolist()), tuple(sorted(self.stats().items())))


def model(origins, dirs, g, cull_eps=R.CULL_EPS, exp_kind=1, variant=None, stale=None):
    """The plan of a bundle.  variant (WRONG, one line each): "long_ge" a list of exactly RAY_PL is queued; "morton_order" the lists stand
    in Morton order; "slot_order" ray r holds the list of the ray in sorted slot r; "stale_queue" the queue is the one of `stale`, another
    plan; "offsets_shifted" the offsets begin one ray late."""
    keep = R.kept(origins, dirs, g, cull_eps, exp_kind)
    lists = [np.nonzero(k)[0] for k in keep]
    if variant == "morton_order":
        rank = np.argsort(X.morton_order(g), kind="stable")                 # scene index -> Morton position
        lists = [l[np.argsort(rank[l], kind="stable")] for l in lists]
    if variant == "slot_order":
        order = RS.sort_order(RS.Spheres(g, origins, dirs, False, cull_eps).keys(1))
        lists = [lists[int(s)] for s in order]
    lens = np.array([len(l) for l in lists], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    if variant == "offsets_shifted":
        offsets = np.concatenate([[0], offsets[:-1]])
    queue = np.nonzero(lens >= RAY_PL if variant == "long_ge" else lens > RAY_PL)[0]
    if variant == "stale_queue":
        queue = stale.queue
    return Plan(offsets, np.concatenate(lists + [np.zeros(0, np.int64)]), queue)


# ---- the bundles of the same-bits tests: a GradScene each (the Gaussians, the rays, d(loss) / d(radiance)) ----
def _scene(name, g, o, d, markers=()):
    o = np.asarray(o, np.float32)
    d = np.asarray(d, np.float32)
    return G.GradScene(name, g, o, d, G.seeded_gr(len(d), 900 + sum(map(ord, name))), markers)


def per_ray_origins(sc):
    """The same bundle with the shared origin given once per ray"""
    assert sc.o.size == 3
    return G.GradScene(sc.name + " per-ray", sc.g, np.ascontiguousarray(np.broadcast_to(sc.o, sc.d.shape)), sc.d, sc.gr, sc.markers)


def first_rays(sc, n):
    return G.GradScene(f"{sc.name} [{n}]", sc.g, sc.o if sc.o.size == 3 else sc.o[:n], sc.d[:n], sc.gr[:n], sc.markers)


def edge_scenes(oracle):
    """The short / long edge (lists of RAY_PL - 1, RAY_PL, RAY_PL + 1 next to rays that keep a few or nothing), the RAY_LCAP edge (the list
    continues in plan memory), ragged last chunks, and a scene of no Gaussians"""
    out = []
    for k in (RAY_PL - 1, RAY_PL, RAY_PL + 1):
        o, d = stack_rays(62)
        out.append(_scene(f"stack {k}", stack_with_side(oracle, k), o, d))
    for n in (RAY_LCAP - 1, RAY_LCAP, RAY_LCAP + 1):
        sc = wide_stack(oracle, RAY_LCAP, n)
        o, d = wide_rays()
        out.append(_scene(f"wide {n}", sc.g, o, d, sc.markers))
    for n in (63, 64, 65, 129):
        g = stack_with_side(oracle, n - 5)
        o, d = stack_rays(62)
        assert len(g) == n
        out.append(_scene(f"ragged {n}", g, o, d))
    o, d = stack_rays(3)
    out.append(_scene("empty", stack(oracle, 4)[:0], o, d))
    return out


def grid_scene(oracle, kind="scattered"):
    """130 rays over the 16 x 16 grid, without the Gaussians whose cull decision float32 could make either way: the model's lists are the
    device's, entry for entry.  "scattered": ray_bundle_scenes.scattered_rays, every ray its own origin, from head-on to grazing along the
    grid's plane -- lists from a handful to far beyond RAY_PL, both kernels in one bundle; "coherent": grad_bundle_scenes' bundle."""
    if kind != "scattered":
        return G.grid_bundle(oracle, kind)
    g0 = oracle.grid_scene(16)
    o, d = scattered_rays(g0, 130)
    return _scene("grid16 scattered", G.settled(g0, o, d), o, d)


def all_scenes(oracle):
    return edge_scenes(oracle) + [grid_scene(oracle, "scattered"), grid_scene(oracle, "coherent")]


# ---- the frozen-list pair ----
NMARK = 8
FROZEN_ORIGIN = np.array([0.0, 0.0, -4.0], np.float32)
FROZEN_S = np.array([2.0, 5.0, 9.0], np.float32)        # in front of the cloud, inside it, behind it


class Frozen:
    """A, B: the same cloud of len(A) Gaussians but for the markers, which stand elsewhere in B.  o, d: the bundle; marker_rays: the rays
    the markers were placed for; enter[i] / leave[i]: the marker that is on marker ray i in B alone / in A alone; stay[i]: the marker
    that moves a little along marker ray i and is kept by it in both."""

    def __init__(self, A, B, o, d, marker_rays, enter, leave, stay):
        self.A, self.B, self.o, self.d, self.marker_rays, self.enter, self.leave, self.stay = A, B, o, d, marker_rays, enter, leave, stay

    def scene(self, which, frozen=False):
        """A GradScene of A or B; frozen: B's Gaussians under A's lists, what a planned call with KEEP_LISTS computes"""
        g = self.A if which == "A" else self.B
        sc = _scene(f"frozen {which}{' under A' if frozen else ''}", g, self.o, self.d, list(self.enter) + list(self.leave) + list(self.stay))
        if frozen:
            keepA = self.scene("A").lists
            sc.lists = lambda cull_eps=1e-9, exp_kind=1: keepA(cull_eps, exp_kind)
        return sc


def in_margin(o, d, g, cull_eps=R.CULL_EPS, exp_kind=1):
    """[N] bool: Gaussians that some ray's float32 cull could decide either way -- within ray_bundle_scenes.kept_range's margin of the
    threshold, under the options the GPU suite runs the pair with"""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    oc = g["mu"][:, :3].astype(np.float64)[None] - o[:, None]
    t = (oc * d[:, None]).sum(2)
    scale = 1.0 / (2.0 * g["sigma"].astype(np.float64) ** 2)[None]
    x = ((oc * oc).sum(2) - t * t) * scale
    band = 8.0 * 2.0 ** -24 * (oc * oc).sum(2) * scale + 1e-5 * np.abs(x)
    return (np.abs(x - G.cull_x_of(g, cull_eps, exp_kind)[None]) <= band).any(0)


def frozen_pair(oracle, n=192, nrays=130, seed=41):
    """A cloud of faint Gaussians in front of the origin and 3 NMARK strong markers behind it in the list.  Marker ray i passes through
    ENTER marker i in B (in A that marker stands far outside every ray's reach) and through LEAVE marker i in A (far outside in B).  A
    call that freezes A's lists on B keeps the LEAVE markers, which shade nothing from where they now stand, and never sees the ENTER
    markers: it differs from B's own sum by the ENTER markers' radiance and absorption.  STAY marker i moves by a few hundredths on
    marker ray i and is kept by it in A and in B: the part of B - A that a derivative under A's lists responds to.  Gaussians whose cull decision float32 could make
    either way on A or on B are taken out (at most 5 % of the draw)."""
    rng = np.random.default_rng(seed)
    mu = np.concatenate([rng.uniform(-0.8, 0.8, size=(n, 2)), rng.uniform(0.6, 1.4, size=(n, 1))], 1)
    sigma = rng.uniform(0.05, 0.1, n)
    mag = rng.uniform(0.2, 0.5, n)
    alb = rng.uniform(0.1, 1.0, size=(n, 4))
    target = np.concatenate([rng.uniform(-0.7, 0.7, size=(nrays, 2)), np.ones((nrays, 1))], 1)
    d = R.normalise(target - FROZEN_ORIGIN.astype(np.float64))
    marker_rays = np.sort(rng.choice(nrays, NMARK, replace=False))
    on_ray = lambda r, t: FROZEN_ORIGIN.astype(np.float64) + t * d[r].astype(np.float64)      # noqa: E731
    far = lambda i, side: np.array([6.0 + i, side * 6.0, 1.0])                                  # noqa: E731
    m_mu_A = np.array([far(i, 1.0) for i in range(NMARK)] + [on_ray(r, 5.3) for r in marker_rays] + [on_ray(r, 5.0) for r in marker_rays])
    m_mu_B = np.array([on_ray(r, 4.7) for r in marker_rays] + [far(i, -1.0) for i in range(NMARK)]
                      + [on_ray(r, 5.04) + [0.01, -0.02, 0.0] for r in marker_rays])
    m_sigma, m_mag = np.full(3 * NMARK, 0.06), np.full(3 * NMARK, 3.0)
    m_alb = np.tile(np.array([[1.0, 0.4, 0.2, 1.0], [0.2, 1.0, 0.4, 1.0], [0.4, 0.2, 1.0, 1.0]]), (NMARK, 1))
    A = oracle.gaussians(np.concatenate([alb, m_alb]), np.concatenate([mu, m_mu_A]), np.concatenate([sigma, m_sigma]), np.concatenate([mag, m_mag]))
    B = oracle.gaussians(np.concatenate([alb, m_alb]), np.concatenate([mu, m_mu_B]), np.concatenate([sigma, m_sigma]), np.concatenate([mag, m_mag]))
    u = in_margin(FROZEN_ORIGIN, d, A) | in_margin(FROZEN_ORIGIN, d, B)
    assert u.sum() <= 0.05 * len(A) and not u[n:].any(), (int(u.sum()), len(A), np.nonzero(u)[0])
    A, B = A[~u], B[~u]
    first = len(A) - 3 * NMARK
    return Frozen(A, B, FROZEN_ORIGIN, d, marker_rays, np.arange(first, first + NMARK), np.arange(first + NMARK, first + 2 * NMARK),
                  np.arange(first + 2 * NMARK, first + 3 * NMARK))


def list_radiance(oracle, o, d, g, lists, rays, exp_kind=1, erf_kind=1):
    """oracle.radiance of every ray in `rays` over the rows lists[r] of g alone.  [len(rays), 4]"""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    return np.stack([oracle.radiance(o[r if len(o) > 1 else 0], np.asarray(d, np.float32)[r], g[lists[r]], exp_kind, erf_kind) if len(lists[r])
                     else np.zeros(4, np.float32) for r in rays])


def list_T(oracle, o, d, s, g, lists, rays, exp_kind=1, erf_kind=1):
    """oracle.transmittance at the samples s [ns] of every ray in `rays` over the rows lists[r] of g alone.  [len(rays), ns]"""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    return np.stack([oracle.transmittance(o[r if len(o) > 1 else 0], np.asarray(d, np.float32)[r], np.asarray(s, np.float32), g[lists[r]], exp_kind, erf_kind)
                     for r in rays])


def frozen_worth(oracle, fz):
    """Per marker ray what the list difference is worth on B: (|L over A's lists - L over B's lists| max over the channels, the same of
    T max over FROZEN_S, the radiance tolerance of the ray, its transmittance tolerance)"""
    la, lb = fz.scene("A").lists(), fz.scene("B").lists()
    rays = fz.marker_rays
    dL = np.abs(list_radiance(oracle, fz.o, fz.d, fz.B, la, rays).astype(np.float64) - list_radiance(oracle, fz.o, fz.d, fz.B, lb, rays)).max(1)
    dT = np.abs(list_T(oracle, fz.o, fz.d, FROZEN_S, fz.B, la, rays).astype(np.float64) - list_T(oracle, fz.o, fz.d, FROZEN_S, fz.B, lb, rays)).max(1)
    tolL, tolT = frozen_tolerances(oracle, fz)
    return dL, dT, tolL[rays], tolT[rays]


def frozen_tolerances(oracle, fz):
    """ray_bundle_scenes.tolerance and transmittance_bundle_scenes.tolerance of every ray for a sum over A's lists: the kernel that shades
    a ray goes by the length of A's list, the peak is B's under those lists"""
    import transmittance_bundle_scenes as TB
    lo, hi = R.kept_range(fz.o, fz.d, fz.A)
    la = fz.scene("A").lists()
    peak = float(np.abs(list_radiance(oracle, fz.o, fz.d, fz.B, la, range(len(fz.d)))).max())
    return R.tolerance(lo, hi, peak), TB.tolerance(lo, hi, len(fz.A))
