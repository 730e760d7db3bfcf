"""The scenes of the block kernel's suite (tests/block_scenes.py, rendered by tests/test_gpu_block.py) can see what they are for --
properties of the float64 model and of the oracle alone, checked on the CPU with the same builders, plans and pixels as the GPU
test: no level above the lane drops what a lane would keep, the model is sure of every ray (family 3: of 95 % of them), what the
prune drops shows in the image at cull_eps = 1e-7, the budget-edge sums straddle the budget by more than the interval's width, tied
entries are tied in float32 too.
"""
import numpy as np
import pytest

import block_scenes as S
from block_scenes import AMB, GONE, KEPT

IDS = [c.name + (f"-eps{c.eps:g}" if c.eps != S.EPS_TEST else "") for c in S.CASES]


def test_the_budget_by_hand():
    assert S.budget(6.0, 10) == 8192.0 and S.budget(1.0, 10) == pytest.approx(1365.3334) and S.budget(60.0, 10) == 81920.0
    assert S.budget(6.0, 8192) == 16384.0 and S.budget(6.0, 4096) == 8192.0           # max(1, n / 4096)
    assert S.budget(6.0, 10, albedo_scale=4.0) == 2048.0
    assert S.budget(6.0, 10, ref_n=0.0) == 8192.0                                     # no level slack, and still 4096 / 3
    assert S.budget(6.0, 10, eps=0.0) == 0.0
    g = np.zeros(2, [("albedo", np.float32, 4)])
    g["albedo"][0] = (0.5, -4.0, np.inf, 1.0)
    assert S.albedo_scale(g) == 4.0 and S.albedo_scale(g[1:]) == 1.0


def test_the_interval_by_hand():
    """t = 9: biased to 9.0091, fp16 spacing in [8, 16) is 2^-7, so the stored value lies within 9.0091 (1 +- 2^-11); the width of
    the interval in e is 2 x 9.0091 x 2^-11 = 0.88 %, and the true value is always below the interval (the bias is what makes the
    prune's sum an upper bound)."""
    lo, hi = S.ln_e_interval(9.0)
    assert lo > 9.0 and lo == pytest.approx(9.0091 * (1 - 2.0 ** -11), abs=1e-4) and hi == pytest.approx(9.0091 * (1 + 2.0 ** -11), abs=1e-4)
    assert S.width(9.0) == pytest.approx(0.0088, abs=2e-4)
    assert 0.02 < S.edge_margin(8192.0) < 0.03
    for t in (0.0, 1e-3, 0.5, 5.0, 9.0, 30.0, 80.0):                  # the fp16 value of the biased t, as numpy rounds it
        h = float(np.float16(np.float32(t) + np.float32(0.001) * abs(np.float32(t)) + np.float32(1e-4)))
        lo, hi = S.ln_e_interval(t)
        assert lo <= h <= hi and t < h


def restated(e, present, floor, budget):
    """prune_list in plain loops over exact values: which of the present entries go."""
    gone = []
    for k in range(len(e)):
        below = sum(e[l] for l in range(len(e)) if present[l] and not floor[l] and e[l] <= e[k])
        gone.append(bool(present[k] and not floor[k] and below <= budget))
    return gone


@pytest.mark.parametrize("key,eps", [(("factors", "plain"), S.EPS_TEST), (("ragged", "both"), S.EPS_TEST), (("ties", 3, False), S.EPS_TEST),
                                     (("floor",), 1e-38)], ids=["factors", "ragged", "ties", "floor"])
def test_the_plan_restates_the_rule(oracle, key, eps):
    """The plan's vectorised brackets against the rule in plain loops, evaluated at the middle of every interval: wherever the
    plan is sure, the two agree, ray by ray and entry by entry."""
    sc = S.scene(oracle, key)
    p, G = S.plan(sc, eps, S.KAPPA), S.geometry(sc, eps)
    sure = 0
    for b in p.blocks:
        slack = np.log(S.REF_N / max(b.cnt, 1))
        for pix in b.lanes:
            j = b.survivors
            thr = np.where(G.floor[j], G.cull_x[j], G.cull_x[j] - slack)
            present = ~(G.x[pix, j] > thr)
            lo, hi = S.ln_e_interval(G.cull_x[j] - G.x[pix, j])
            gone = restated(np.exp(0.5 * (lo + hi)), present, G.floor[j], p.budget) if present.sum() <= S.PRUNE_PL else [False] * len(j)
            for k, jj in enumerate(j):
                want = GONE if gone[k] else (KEPT if present[k] else S.ABSENT)
                if p.status[pix, jj] != AMB:
                    assert p.status[pix, jj] == want, (pix, jj)
                    sure += 1
    assert sure > 0.9 * sum(64 * b.cnt for b in p.blocks)


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_levels_and_ambiguity(oracle, c):
    """No cone or tile decision within its margin, no level above the lane drops what a lane would keep, every block is the block
    kernel's (cnt <= 96, lists <= 24: asserted by the plan); the model is sure of every ray, or of 95 % in family 3, where a
    budget crossing inside a block must leave some open."""
    sc = S.scene(oracle, c.key)
    for kappa in {c.kappa, 0.0}:
        p = S.plan(sc, c.eps, kappa)
        assert p.cone_unsure == 0 and p.above_drops == 0
        assert p.n_blocks == (sc.w // 8) * (sc.h // 8) and all(b.cnt >= 1 for b in p.blocks)
        if c.exact or kappa == 0.0:
            assert p.n_ambiguous == 0 and p.lane_entries[0] == p.lane_entries[1] and p.lane_pairs[0] == p.lane_pairs[1]
        else:
            assert p.n_ambiguous <= S.AMBIGUOUS_MAX * sc.w * sc.h
            assert all((~p.ambiguous[b.lanes]).any() for b in p.blocks)
    if sc.n > 1000:      # the large scene: the model's tile set is the reference's
        tiles = oracle.tile_gaussians(2.0, 2.0, sc.g, sc.view)
        assert tiles["w"] == tiles["h"] == 1
        kept = np.flatnonzero((S.plan(sc, c.eps, c.kappa).status != S.ABSENT).any(0))
        assert set(kept) <= set(tiles["indices"][:tiles["offsets"][1]]) and tiles["offsets"][1] == S.plan(sc, c.eps, c.kappa).tile_entries // 4


def test_what_each_family_is_built_to_show(oracle):
    """The decisions the scenes are for, read from the model: counts per family."""
    for k, side, pos in [c[1:] for c in S.EDGE_CASES]:
        sc = S.scene(oracle, ("edge", k, side, pos))
        p = S.plan(sc)
        G = S.geometry(sc, S.EPS_TEST)
        assert p.n_pruned == 256 * sc.expect_dropped
        big = sc.faint_at[-1]
        assert (p.status[:, sc.faint_at[:-1]] == GONE).all() and (p.status[:, big] == (GONE if side < 0 else KEPT)).all()
        # the two sums straddle the budget by more than the interval's width
        lo, hi = S.ln_e_interval(G.cull_x[sc.faint_at][None, :] - G.x[:, sc.faint_at])
        w = S.width(np.log(p.budget))
        if side < 0:
            assert (np.exp(hi).sum(1) * (1 + w) <= p.budget).all()
        else:
            assert (np.exp(lo).sum(1) > p.budget * (1 + w)).all() and (np.exp(hi)[:, :-1].sum(1) * (1 + w) <= p.budget).all()
    lefts = set()
    for _, nmax, pos in S.INST_CASES:
        p = S.plan(S.scene(oracle, ("inst", nmax, pos)))
        assert all(b.nmax == (nmax, nmax) for b in p.blocks)
        assert p.n_pruned == (256 if nmax <= S.PRUNE_PL else 0) and p.n_kept == 256 * (nmax - 1 if nmax <= S.PRUNE_PL else nmax)
        lefts |= {b.left[0] for b in p.blocks}
    assert lefts == set(range(16)) | {17} and {n % 4 for n in lefts} == {0, 1, 2, 3}
    for kind in ("narrow", "both"):                         # lanes of one block with lists of different lengths, inside one template
        p = S.plan(S.scene(oracle, ("ragged", kind)))
        nl = ((p.status == KEPT) | (p.status == GONE) | (p.status == AMB)).sum(1)
        assert any(nl[b.lanes].min() < nl[b.lanes].max() <= S.PRUNE_PL for b in p.blocks)
    for kind in ("cross", "both"):                          # neighbours in one block: some lanes drop the entry, some keep it
        sc = S.scene(oracle, ("ragged", kind))
        p = S.plan(sc)
        j = sc.faint_at[0]
        assert all((p.status[b.lanes, j] == GONE).any() and (p.status[b.lanes, j] == KEPT).any() for b in p.blocks)
        assert 0 < p.n_ambiguous
    for copies, fit in [c[1:] for c in S.TIE_CASES]:
        sc = S.scene(oracle, ("ties", copies, fit))
        p = S.plan(sc)
        assert (p.status[:, sc.faint_at[0]] == GONE).all() and (p.status[:, sc.tied] == (GONE if fit else KEPT)).all()
    p = S.plan(S.scene(oracle, ("nothing", "none")))
    assert p.n_pruned == 0
    sc = S.scene(oracle, ("nothing", "one-lane"))
    p = S.plan(sc)
    assert p.n_pruned == 1 and p.status[sc.lane_pixel, sc.n - 1] == GONE and (np.delete(p.status[:, sc.n - 1], sc.lane_pixel) == S.ABSENT).all()
    sc = S.scene(oracle, ("lane",))
    p = S.plan(sc, kappa=0.0)
    assert [b.cnt for b in p.blocks] == [8, 9, 9, 9] and all(b.n_list == 11 for b in p.blocks)
    over, under = sc.faint_at
    assert (p.status[:, over] == KEPT).all() and (p.status[p.blocks[0].lanes, under] == S.ABSENT).all()
    assert all((p.status[b.lanes, under] == KEPT).all() for b in p.blocks[1:])
    sc = S.scene(oracle, ("factors", "plain"))
    for kappa, drops in S.FACTOR_DROPS.items():
        assert S.plan(sc, kappa=kappa).n_pruned == 256 * drops
    assert S.plan(sc, ref_n=0.0).n_pruned == 256 * 4 and S.plan(sc, ref_n=0.0).budget == 8192.0
    for key in (("factors", "plain"), ("lane",)):                   # the frames of the context without level slack
        for kappa in (S.KAPPA, 0.0):
            p = S.plan(S.scene(oracle, key), kappa=kappa, ref_n=0.0)
            assert p.n_ambiguous == 0 and p.cone_unsure == 0 and p.above_drops == 0
    assert S.plan(S.scene(oracle, ("factors", "albedo4"))).n_pruned == 256 * 2 == S.plan(S.scene(oracle, ("factors", "albedo-inf"))).n_pruned
    assert S.plan(S.scene(oracle, ("factors", "negative"))).n_pruned == 256 * 4
    large = S.scene(oracle, ("factors", "large"))
    assert large.n == 8192 and S.plan(large).budget == 16384.0 and S.plan(large).n_pruned == 256 * 4
    assert S.plan(large, kappa=3.0).n_pruned == 256 * 3            # half the budget: what a missing n / 4096 would give
    sc = S.scene(oracle, ("floor",))
    p, G = S.plan(sc, 1e-38), S.geometry(sc, 1e-38)
    assert list(G.floor) == [True, True, False, False, False]
    small = np.exp(G.cull_x[None, :2] - G.x[:, :2]) < p.budget / 10          # floor entries far below the budget ...
    assert ((p.status[:, :2] == KEPT) & small).sum() > 50 and not (p.status[:, :2] == GONE).any()      # ... stay
    assert (p.status[:, 2:4] == GONE).sum() > 50 and (p.status[:, 2:4] == KEPT).sum() > 50


@pytest.mark.parametrize("c", [c for c in S.CASES if c.marked], ids=[c.name for c in S.CASES if c.marked])
def test_the_dropped_set_shows(oracle, c):
    """At cull_eps = 1e-7 leaving out what the model says the prune drops moves a checked pixel by at least MARKER_FACTOR
    tolerances of the GPU test, and by no more than the documented bound, 3 budget eps_eff."""
    sc = S.scene(oracle, c.key)
    p1, rad1, _, pix = S.reference(oracle, sc, c.eps, c.kappa)
    _, rad0, _, _ = S.reference(oracle, sc, c.eps, 0.0)
    tol = S.TOL_NOCULL * max(1.0, float(rad0[pix].max()))
    moved = np.abs(rad1 - rad0)[pix].max(1)
    assert moved.max() >= S.MARKER_FACTOR * tol, moved.max()
    assert moved.max() <= 3.0 * p1.budget * S.geometry(sc, c.eps).eps_eff


def test_tied_entries_are_tied_in_float32(oracle):
    """Bit-identical rows; and x, formed in float32 operation by operation as the lane cull does, is the same bits on every ray."""
    f = np.float32
    for copies, fit in [c[1:] for c in S.TIE_CASES]:
        sc = S.scene(oracle, ("ties", copies, fit))
        rows = sc.g[sc.tied]
        assert all(r.tobytes() == rows[0].tobytes() for r in rows) and len(rows) == copies
        assert len(set(S.geometry(sc, S.EPS_TEST).group[sc.tied])) == 1
        o = sc.origin.astype(f)
        p = np.stack([np.asarray(a, f) for a in sc.plane], 1) - o
        nrm = np.sqrt(((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]).astype(f) + p[:, 2] * p[:, 2]).astype(f)).astype(f)
        d = (p / nrm[:, None]).astype(f)
        xs = []
        for j in sc.tied:
            a = sc.g["mu"][j, :3].astype(f) - o
            aw = ((a[0] * a[0] + a[1] * a[1]).astype(f) + a[2] * a[2]).astype(f)
            mubar = ((a[0] * d[:, 0] + a[1] * d[:, 1]).astype(f) + a[2] * d[:, 2]).astype(f)
            s = f(sc.g["sigma"][j])
            xs.append(((aw - (mubar * mubar).astype(f)).astype(f) * (f(1) / (f(2) * s * s))).astype(f))
        assert all((x.view(np.uint32) == xs[0].view(np.uint32)).all() for x in xs)


def test_tie_stacks_are_one_entry_k_times(oracle):
    """The scenes of the bit-exact budget test: k identical entries and nothing else, kept by every ray under cull_ref_n = 1024 (a
    power of two: every fp32 budget is then kappa x 1024 for an fp32 kappa), and the same x on every ray whatever k."""
    x1 = S.geometry(S.scene(oracle, ("stack", 1)), S.EPS_TEST).x[:, 0]
    for k in range(1, S.PRUNE_PL + 1):
        sc = S.scene(oracle, ("stack", k))
        G = S.geometry(sc, S.EPS_TEST)
        assert sc.n == k and len(set(G.group)) == 1 and all(r.tobytes() == sc.g[0].tobytes() for r in sc.g)
        assert (G.x == x1[:, None]).all()
        p = S.plan(sc, S.EPS_TEST, 0.0, 1024.0)
        assert p.n_ambiguous == 0 and p.cone_unsure == 0 and p.n_kept == 256 * k
    assert float(S.running_sum32(3.0, 3)) == 9.0 and S.running_sum32(np.float32(1.0) + np.float32(2.0 ** -23), 3) == np.float32(3.0) + np.float32(2.0 ** -21)
