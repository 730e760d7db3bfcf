"""The one-wave block kernel (csrc/vrt_block_kernel.hip: render_body) on its own: the lane cull with the block's survivor count in
its threshold, and the budgeted prune (prune_list) decision by decision -- the budget's edge from both sides, every instantiation
of the `switch (nmax)`, lanes of one block with lists of different lengths, tied entries, the early exit, the budget's factors
(kappa, the albedo scale, |sigma mag|, n / 4096, VRT_HIP_CULL_REF_N=0) and entries at the Exp floor.  Scenes, the float64 model of
the per-ray decisions and the intervals it derives: tests/block_scenes.py; that the scenes can see what they are for:
tests/test_block_scenes.py.  The capacity limits (PL, PRUNE_PL) stay with tests/test_gpu_boundaries.py.

Every frame is one tile and one 32x32 cell, Exp VCL / Erf A&S, exact kernels (table step 0), statistics on.  Most run at cull_eps =
1e-7: the kernel decides in units of e / eps, so its decisions are those of the default 1e-9, and what the prune drops is then worth
up to 2.5e-3 in radiance, a hundred tolerances.  Per frame:
  lists       dense_blocks == 0, shaded_blocks, tile_entries and list_entries are the model's (no level above the lane interferes)
  statistics  lane_entries, lane_pairs and lane_max_entries -- all counted after the prune -- EQUAL the model's counts wherever the
              model has no ambiguous ray; in family 3 they lie between its two counts
  radiance    on the unambiguous rays within TOL_NOCULL max(1, peak) of the oracle's sum over the model's kept set of that ray, packed
              pixels within 1
  prune       on against off: at most 3 budget eps_eff (include/vrt_hip.h) on every pixel; in families 1, 2 and 4 at least half of
              what the oracle says the model's dropped set is worth, wherever that is ten tolerances or more
"""
import numpy as np
import pytest

import block_scenes as S

pytestmark = pytest.mark.gpu

STATS = ("lane_entries", "lane_pairs", "lane_max_entries")
IDS = [c.name + (f"-eps{c.eps:g}" if c.eps != S.EPS_TEST else "") for c in S.CASES]


def channels(img):
    img = np.asarray(img).reshape(-1)
    return ((img[:, None] >> np.array([0, 8, 16, 24], np.uint32)) & 255).astype(np.int32)


def load(r, sc):
    r.set_gaussians(sc.g)
    r.set_plane(sc.w, sc.h, *sc.plane)
    r.tile_gaussians(sc.tw, sc.th, sc.view)


def shoot(pkg, r, sc, eps, kappa):
    """One frame with statistics: (packed pixels, radiance in float64 -- the same bits --, statistics)."""
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, eps)
    r.set_table_step(0.0)
    r.set_cull_prune(kappa)
    r.enable_stats(True)
    img, rad = r.render(sc.origin)
    return img.reshape(-1).copy(), rad.reshape(-1, 4).astype(np.float64), r.stats()


def restore(pkg, r):
    r.enable_stats(False)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    r.set_table_step(pkg.TABLE_STEP_DEFAULT)
    r.set_cull_prune(6.0)


def show(what, st):
    keys = ("shaded_blocks", "dense_blocks", "tile_entries", "list_entries") + STATS
    print(what, " ".join(f"{k}={st[k]}" for k in keys), flush=True)


def hold_statistics(what, st, p, exact):
    """Lists and paths, then the three per-ray statistics against the model's counts.  Returns where each sits in its bracket."""
    show(what, st)
    assert st["dense_blocks"] == 0 and st["overflow_blocks"] == 0, what
    assert st["shaded_blocks"] == p.n_blocks, (what, st["shaded_blocks"])
    assert st["tile_entries"] == p.tile_entries and st["list_entries"] == p.list_entries, (what, st["tile_entries"], st["list_entries"])
    where = {}
    for k in STATS:
        lo, hi = p[k]
        if exact:
            assert lo == hi, (what, k)
        assert lo <= st[k] <= hi, (what, k, st[k], (lo, hi))
        where[k] = (st[k] - lo, hi - lo)
    return where


def hold_radiance(what, sc, img, rad, ref):
    p, orad, oimg, pix = ref
    tol = S.TOL_NOCULL * max(1.0, float(orad[pix].max()))
    err = np.abs(rad - orad)[pix].max(1)
    print(f"{what}: largest error against the oracle over the kept sets {err.max():.3g} (tolerance {tol:.3g}) on {len(pix)} rays", flush=True)
    assert (err <= tol).all(), (what, float(err.max()), int(pix[np.argmax(err)]))
    assert np.abs(channels(img[pix]) - channels(oimg[pix])).max() <= 1, what


def run_case(pkg, oracle, r, c, ref_n=S.REF_N):
    sc = S.scene(oracle, c.key)
    what = IDS[S.CASES.index(c)] if c in S.CASES else c.name
    load(r, sc)
    p1 = S.plan(sc, c.eps, c.kappa, ref_n)
    img1, rad1, st1 = shoot(pkg, r, sc, c.eps, c.kappa)
    where = hold_statistics(f"{what}:", st1, p1, c.exact)
    if c.radiance:
        hold_radiance(what, sc, img1, rad1, S.reference(oracle, sc, c.eps, c.kappa, ref_n))
    if c.kappa > 0.0:
        p0 = S.plan(sc, c.eps, 0.0, ref_n)
        img0, rad0, st0 = shoot(pkg, r, sc, c.eps, 0.0)
        hold_statistics(f"{what} prune off:", st0, p0, True)
        moved = np.abs(rad1 - rad0).max(1)
        bound = 3.0 * p1.budget * S.geometry(sc, c.eps).eps_eff
        if np.isfinite(moved).all():
            print(f"{what}: the prune moves a pixel by {moved.max():.3g}, bound {bound:.3g}", flush=True)
            assert moved.max() <= bound, (what, float(moved.max()), bound)
        if c.radiance:
            ref0 = S.reference(oracle, sc, c.eps, 0.0, ref_n)
            hold_radiance(f"{what} prune off", sc, img0, rad0, ref0)
        if c.marked:
            _, orad1, _, pix = S.reference(oracle, sc, c.eps, c.kappa, ref_n)
            worth = np.abs(orad1 - ref0[1])[pix].max(1)
            tol = S.TOL_NOCULL * max(1.0, float(ref0[1][pix].max()))
            tell = worth >= S.MARKER_FACTOR * tol
            assert tell.any(), what
            assert (moved[pix][tell] >= 0.5 * worth[tell]).all(), (what, float((moved[pix][tell] / worth[tell]).min()))
    return sc, (img1, rad1, st1), where


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_decisions(pkg, oracle, renderer, c):
    """Every scene of tests/block_scenes.py under its settings: lists, statistics, radiance and the prune's effect as the module's
    docstring says.  Family 3 (ragged blocks) prints where each statistic sits inside the model's bracket."""
    try:
        sc, _, where = run_case(pkg, oracle, renderer, c)
        if not c.exact:
            print(c.name, "position in the bracket:", " ".join(f"{k} +{a} of {b}" for k, (a, b) in where.items()), flush=True)
    finally:
        restore(pkg, renderer)


def test_an_empty_list_is_exactly_black(pkg, oracle, renderer):
    """nmax = 1, a lone prunable Gaussian: every ray ends with an empty list -- radiance exactly 0 and a pixel of 0 --, and without
    the prune it does not."""
    sc = S.scene(oracle, ("inst", 1, "last"))
    load(renderer, sc)
    try:
        img1, rad1, st1 = shoot(pkg, renderer, sc, S.EPS_TEST, S.KAPPA)
        img0, rad0, _ = shoot(pkg, renderer, sc, S.EPS_TEST, 0.0)
        assert st1["lane_entries"] == 0 and st1["lane_max_entries"] == 0 and st1["shaded_blocks"] == 4
        assert (rad1 == 0.0).all() and (img1 == 0).all()
        assert rad0[:, :3].min() > 0.0
    finally:
        restore(pkg, renderer)


def test_nothing_to_do_is_bit_equal(pkg, oracle, renderer):
    """The `__ballot(least <= budget) == 0` exit, and lists beyond PRUNE_PL: image and radiance bit for bit those of the prune switched
    off.  Four blocks of which one lane of one block has a prunable entry: that pixel differs, every other pixel is the same bits."""
    try:
        for key in (("nothing", "none"), ("inst", 17, "last")):
            sc = S.scene(oracle, key)
            load(renderer, sc)
            img1, rad1, st1 = shoot(pkg, renderer, sc, S.EPS_TEST, S.KAPPA)
            img0, rad0, st0 = shoot(pkg, renderer, sc, S.EPS_TEST, 0.0)
            np.testing.assert_array_equal(img1, img0)
            np.testing.assert_array_equal(rad1, rad0)
            assert all(st1[k] == st0[k] for k in STATS)
        sc = S.scene(oracle, ("nothing", "one-lane"))
        load(renderer, sc)
        img1, rad1, st1 = shoot(pkg, renderer, sc, S.EPS_TEST, S.KAPPA)
        img0, rad0, st0 = shoot(pkg, renderer, sc, S.EPS_TEST, 0.0)
        differs = (rad1 != rad0).any(1)
        assert list(np.flatnonzero(differs)) == [sc.lane_pixel], np.flatnonzero(differs)
        assert st0["lane_entries"] - st1["lane_entries"] == 1 and st0["lane_pairs"] - st1["lane_pairs"] == 7 * 7 - 6 * 6
        assert st0["lane_max_entries"] - st1["lane_max_entries"] == 1
    finally:
        restore(pkg, renderer)


def test_survivors_keep_their_order(pkg, oracle, renderer):
    """The compaction keeps the survivors in list order: the same bright Gaussians with the faint run at the first, a middle and the
    last position give, once the run is gone (side -1: all of it goes), the same per-ray lists -- the same bits."""
    try:
        for k in (1, 2, 3, 5):
            rads = []
            for pos in ("first", "middle", "last"):
                sc = S.scene(oracle, ("edge", k, -1, pos))
                load(renderer, sc)
                rads.append(shoot(pkg, renderer, sc, S.EPS_TEST, S.KAPPA)[1])
            np.testing.assert_array_equal(rads[0], rads[1])
            np.testing.assert_array_equal(rads[0], rads[2])
    finally:
        restore(pkg, renderer)


def test_without_level_slack(pkg, oracle, monkeypatch):
    """A fresh context under VRT_HIP_CULL_REF_N=0: no slack at any level (a lane keeps e >= 1), and the budget still uses 4096 / 3."""
    monkeypatch.setenv("VRT_HIP_CULL_REF_N", "0")
    r = pkg.Renderer(0)
    try:
        for key in (("factors", "plain"), ("lane",)):
            c = S.case(key, kappa=S.KAPPA)
            c["name"] += "-ref_n0"
            sc, _, _ = run_case(pkg, oracle, r, c, ref_n=0.0)
        assert (S.plan(sc, S.EPS_TEST, 0.0, 0.0).status[:, sc.faint_at] == S.KEPT).all()      # the lane scene: without slack both faint entries stay
    finally:
        r.close()


def first_drop(pkg, r, sc, lo, hi):
    """The smallest fp32 budget at which the frame loses an entry, by bisection over the bit patterns between lo (nothing goes) and
    hi (something does).  The context's cull_ref_n is 1024, so budget = kappa x 1024 exactly."""
    full = sc.n * sc.w * sc.h

    def drops(bits):
        r.set_cull_prune(float(np.uint32(bits).view(np.float32)) / 1024.0)
        r.render(sc.origin, want_radiance=False)
        return r.stats()["lane_entries"] < full

    lo, hi = int(np.float32(lo).view(np.uint32)), int(np.float32(hi).view(np.uint32))
    assert not drops(lo) and drops(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if drops(mid) else (mid, hi)
    return np.uint32(hi).view(np.float32)


def test_the_budget_is_met_to_the_bit(pkg, oracle, monkeypatch):
    """"Entry k goes iff the sum of all entries not larger than it FITS": `<=`, to the last bit.  k bit-identical entries (k = 1 ..
    16: every instantiation again) and nothing else; b_k is the smallest fp32 budget at which the frame loses an entry, found by
    bisection.  b_1 is the smallest e of the frame as the kernel holds it -- inside the model's interval --, and with `<=` b_k is
    exactly b_1 + b_1 + ... in fp32, left to right, as prune_list adds them.  With `below < budget` every b_k is one ulp higher, and
    a sum of k numbers that are one ulp higher is not one ulp higher for every k (for k = 3 it is 1.5 or 0.75 ulps of the sum)."""
    monkeypatch.setenv("VRT_HIP_CULL_REF_N", "1024")
    r = pkg.Renderer(0)
    try:
        r.set_options(pkg.EXP_VCL, pkg.ERF_AS, S.EPS_TEST)
        r.set_table_step(0.0)
        r.enable_stats(True)
        b = {}
        for k in range(1, S.PRUNE_PL + 1):
            sc = S.scene(oracle, ("stack", k))
            load(r, sc)
            G = S.geometry(sc, S.EPS_TEST)
            lo, hi = S.ln_e_interval(G.cull_x[0] - G.x[:, 0], G.err_x[:, 0] + G.err_cull[0])
            b[k] = first_drop(pkg, r, sc, 0.9 * k * 3000.0, 1.1 * k * 3000.0)
            print(f"k={k}: first drop at a budget of {b[k]!r}, the model's interval [{k * np.exp(lo.min()):.8g}, {k * np.exp(hi.min()):.8g}]", flush=True)
            assert k * np.exp(lo.min()) * (1 - S.ERR_SUM) <= b[k] <= k * np.exp(hi.min()) * (1 + S.ERR_SUM)
        for k in b:
            assert b[k] == S.running_sum32(b[1], k), (k, b[k], S.running_sum32(b[1], k))
    finally:
        r.close()
