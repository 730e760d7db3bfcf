"""The table kernel's cases (tests/table_cases.py, rendered by tests/test_gpu_table.py) sit where they are meant to sit and can see
what they are meant to see -- properties of the float64 model (tests/table_scenes.py) and of the reference alone, checked on the
CPU with the same builders, steps, budgets and pixels as the GPU test.
"""
import numpy as np
import pytest

import boundary_scenes as B
import table_cases as TC
import table_scenes as T

WAVES = (16, 8)


def tolerance(c, dw, peak):
    """What the GPU test allows between the table frame and the exact one: the case's budget and the fp32 noise term."""
    return TC.budget(c, dw) + T.NOISE * max(1.0, peak)


def planned(oracle, dw):
    """The cases whose plan is the requested one (VRT_HIP_TABLE_ADAPT=1): all but the retry and coarsening cases."""
    return [c for c in TC.cases(oracle, dw) if c.kind in ("table", "decline", "exact-pair")]


def test_plan_restates_the_kernel_by_hand():
    # 16 waves: 376 intervals per segment at most, 56 in the smallest table; 8 waves: 184 and 24
    assert T.plan_of_need(56, 16) == (1, 4) and T.plan_of_need(57, 16) == (1, 6) and T.plan_of_need(376, 16) == (1, 24)
    assert T.plan_of_need(377, 16) == (2, 16) and T.plan_of_need(3007, 16) == (8, 24) and T.plan_of_need(3008, 16) is None
    assert T.plan_of_need(24, 8) == (1, 4) and T.plan_of_need(25, 8) == (1, 6) and T.plan_of_need(184, 8) == (1, 24)
    assert T.plan_of_need(185, 8) == (2, 16) and T.plan_of_need(1471, 8) == (8, 24) and T.plan_of_need(1472, 8) is None
    assert T.margin_of_need(56, 16) == 0 and T.margin_of_need(54, 16) == 2 and T.margin_of_need(3010, 16) == 2
    nseg, nt, sl, g, gtot, h, u = T.plan(10.0, 2.0, 0.05, 16)               # need 400: two segments of 200 -> NT 16, SL 248
    assert (nseg, nt, sl, g, gtot) == (2, 16, 248, 256, 502) and h == pytest.approx(10.0 / 496 * 1.00001) and u == pytest.approx(2.0 * h)
    assert T.plan(10.0, 2.0, 1.0, 16) is None                               # 20 intervals in a table of 56: u = 20 / 56 > 0.3
    assert T.plan(10.0, 2.0, 0.006, 16) is None                             # 3334 intervals: more than eight segments


@pytest.mark.parametrize("dw", WAVES)
def test_menu_margin(oracle, dw):
    """Every planned case is at least two intervals from the nearest edge of the menu in every block, and its spacing clear of the
    0.3 the error constants hold for: the fp32 kernel and the float64 model cannot disagree about the plan."""
    for c in planned(oracle, dw):
        m = T.menu_margin(c.sc, c.hx, dw)
        plans = T.block_plans(c.sc, c.hx, dw)
        print(f"waves={dw} {c.group}/{c.name}: step {c.hx:.5g} needs {T.block_needs(c.sc, c.hx)} margin {m}")
        assert m >= 2, (c.group, c.name, m)
        if c.kind == "decline":
            assert all(p is None for p in plans) and min(T.block_needs(c.sc, c.hx)) >= T.need_limit(dw)
        else:
            assert all(p is not None and p[6] <= 0.29 for p in plans), (c.group, c.name)
            assert 0.0 < c.hx <= 1.0


@pytest.mark.parametrize("dw", WAVES)
def test_menu_coverage(oracle, dw):
    """Per shape the menu cases select every NT with one segment within three intervals of either end of its band (two is the
    margin; the first band starts at what the largest step gives), two, three and eight segments, and one need beyond the limit.
    At least one case tells the two shapes apart by its node count alone."""
    menu = {c.name: c for c in TC.menu_cases(oracle, dw)}
    for nt, lo, hi in T.bands(dw):
        for end in ("lo", "hi"):
            c = menu[f"NT{nt}-{end}"]
            needs = T.block_needs(c.sc, c.hx)
            assert all(p[:2] == (1, nt) for p in T.block_plans(c.sc, c.hx, dw)), (nt, end)
            if end == "hi":
                assert hi - 3 <= max(needs) <= hi - 2
            elif nt == 4:
                assert c.hx == 1.0
            else:
                assert lo + 2 <= min(needs) <= lo + 3
    for nseg in (2, 3, 8):
        c = menu[f"seg{nseg}"]
        assert all(p[0] == nseg for p in T.block_plans(c.sc, c.hx, dw)), nseg
    assert T.seg_max(dw) + 1 <= min(T.block_needs(menu["seg2"].sc, menu["seg2"].hx)) <= T.seg_max(dw) + 4     # just past one segment
    assert T.need_limit(dw) - 4 <= max(T.block_needs(menu["seg8"].sc, menu["seg8"].hx)) < T.need_limit(dw)   # just before the limit
    c = menu["beyond"]
    assert all(p is None for p in T.block_plans(c.sc, c.hx, dw)) and min(T.block_needs(c.sc, c.hx)) <= T.need_limit(dw) + 4
    assert len(menu) == 2 * len(T.NT_MENU) + 4
    other = 24 - dw
    differ = [c.name for c in menu.values() if c.kind == "table" and T.expected_nodes(c.sc, c.hx, dw) != T.expected_nodes(c.sc, c.hx, other)]
    print(f"waves={dw}: node counts that the other shape would not give: {differ}")
    assert differ


@pytest.mark.parametrize("dw", WAVES)
def test_marker_condition(oracle, dw):
    """Every ray sees the whole scene, and leaving out any one marker moves a checked pixel by at least ten times the tolerance the
    GPU test applies to the case (per scene: the largest tolerance of the cases that render it)."""
    worst = {}
    for c in TC.cases(oracle, dw):
        if c.kind in ("table", "retry", "coarsen"):
            worst.setdefault(c.key, []).append(c)
    for key, cs in worst.items():
        sc = cs[0].sc
        assert B.all_rays_see_all(sc), key
        assert sc.n > B.PL and len(sc.g) == sc.n                        # every ray's list is beyond the block kernel's: the dense path
        effects, peak = B.marker_effects(oracle, sc, threads=8)
        # (the retry case's widest budget is its ladder's top rung)
        tol = max(T.bound_ceiling(c.sc, c.hx, dw, c.erf, adapt=T.ADAPT_DEFAULT) + T.NOISE * max(1.0, peak) if c.kind == "retry"
                  else tolerance(c, dw, peak) for c in cs)
        tol = max(tol, max(max(B.TOL, TC.budget(c, dw)) * max(1.0, peak) for c in cs))     # ... and the one against the oracle
        print(f"waves={dw} {key}: peak {peak:.3f} markers {sc.markers} smallest effect {min(effects.values()):.3g} "
              f"against tolerance {tol:.3g} (x{min(effects.values()) / tol:.0f})")
        assert peak > 0.05
        for k, e in effects.items():
            assert e >= B.MARKER_FACTOR * tol, (key, k, e, tol)


@pytest.mark.parametrize("dw", WAVES)
def test_straddlers_and_skip_bounds(oracle, dw):
    """Every multi-segment case of the depth stacks has, on every checked pixel, a marker whose five samples fall into two
    segments and a marker whose kink lies within one interval of a segment border; every multi-segment case has saturated visits,
    and the two bounds of their count are ordered (everywhere)."""
    seen = 0
    for c in planned(oracle, dw):
        if c.kind != "table":
            continue
        lo, hi = T.skip_bounds(c.sc, c.hx, dw, c.erf)
        assert 0 <= lo <= hi, (c.group, c.name)
        if T.block_plans(c.sc, c.hx, dw)[0][0] > 1:
            assert lo > 0, (c.group, c.name)
            assert hi - lo <= 0.01 * hi                                 # the bounds are no formality
            if c.key[0] == "deep":
                emit, kink = T.straddlers(c.sc, c.hx, dw)
                print(f"waves={dw} {c.group}/{c.name}: straddling emitters {emit} border kinks {kink} skips {lo}..{hi}")
                assert emit and kink, (c.group, c.name)
                seen += 1
    assert seen >= 3


def test_bound_ceilings_at_the_default_step(oracle):
    """For the record (no assertion beyond their order): the ceilings of the cases at the default step beside the default budget."""
    for dw in WAVES:
        for c in TC.cases(oracle, dw):
            if c.hx == T.STEP_DEFAULT:
                a, b = T.bound_ceiling(c.sc, c.hx, dw, c.erf), T.bound_ceiling(c.sc, c.hx, dw, c.erf, adapt=T.ADAPT_DEFAULT)
                print(f"waves={dw} {c.group}/{c.name} n={c.sc.n}: ceiling {a:.3g}, with a first attempt up to 3 x coarser {b:.3g}; "
                      f"default budget {T.BUDGET_DEFAULT:.3g}")
                assert 0.0 < a <= b


@pytest.mark.parametrize("dw", WAVES)
def test_retry_ladder(oracle, dw):
    """The ladder starts at a ceiling that holds whatever the first attempt coarsens to, halves, and ends at 1e-9 -- below what any
    lit ray can meet: the saturation term alone, 1.01 S eps sum amax |term|, is beyond it on a ray of every block."""
    c = next(c for c in TC.cases(oracle, dw, ("retry",)))
    ladder = TC.retry_ladder(c, dw)
    assert ladder[0] == T.bound_ceiling(c.sc, c.hx, dw, c.erf, adapt=T.ADAPT_DEFAULT) >= T.bound_ceiling(c.sc, c.hx, dw, c.erf)
    assert ladder[-1] == 1e-9 and all(b == 0.5 * a for a, b in zip(ladder[:-1], ladder[1:-1])) and 0.5 <= ladder[-1] / ladder[-2] < 1.0
    assert T.block_plans(c.sc, c.hx, dw)[0][0] > 1                      # a multi-segment scene at the default step
    _, orad = B.render_oracle(oracle, c.sc, pixels=np.arange(c.sc.w * c.sc.h, dtype=np.uint32), threads=8)
    G = T._geometry(c.sc)
    # amax <= 1 here, so sum amax |term| >= the largest channel of the radiance
    floor = 1.01 * np.abs(G.A).sum(1) * T.table_saturation_eps(c.erf) * orad.max(1)
    assert min(floor[b].max() for b in G.blocks) > 10 * 1e-9               # one ray over the budget declines its block
