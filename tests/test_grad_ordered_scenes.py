"""CPU checks of tests/grad_ordered_scenes.py: the model of the ordered reduction is a sum within the depth bound it documents, the
crafted record sets tell the normative order from four others, and the aimed bundle stays under `settled`'s cap."""
import numpy as np
import pytest

import grad_bundle_scenes as G
import grad_ordered_scenes as S


@pytest.fixture(scope="module")
def crafted_sets():
    return [S.crafted(seed) for seed in (1, 2, 3)]


def test_segments_are_the_lengths_asked_for(crafted_sets):
    for gauss, rows, n in crafted_sets:
        segs = S.segments(gauss)
        assert tuple(hi - lo for _, lo, hi in segs) == S.SEGMENTS
        assert len({j for j, _, _ in segs}) == len(segs) and max(j for j, _, _ in segs) < n
        assert rows.shape == (len(gauss), S.NREC) and (rows < 0).any() and (rows > 0).any()
        mag = np.abs(rows[rows != 0])
        assert mag.max() / mag.min() > 1e6                      # mixed magnitudes: an order of summation shows


@pytest.mark.parametrize("cols", [S.RADIANCE_COLS, S.TRANS_COLS])
def test_model_agrees_with_the_float64_sum_within_its_depth(crafted_sets, cols):
    for gauss, rows, n in crafted_sets:
        zero = np.zeros((n, S.STRIDE), np.float32)
        got = S.ordered_reduce(gauss, rows, zero, cols)
        for j, lo, hi in S.segments(gauss):
            seg = rows[lo:hi][:, list(cols)].astype(np.float64)
            err = np.abs(got[j, list(cols)].astype(np.float64) - seg.sum(0))
            bound = (S.depth(hi - lo)) * 2.0 ** -24 * np.abs(seg).sum(0)
            assert (err <= bound).all(), (j, hi - lo, err, bound)
            assert (err <= S.sum_bound(hi - lo, np.abs(seg).sum(0))).all()
        assert S.depth(1) == 7 and S.depth(64) == 7 and S.depth(65) == 8 and S.depth(4096) == 70


def test_model_leaves_the_other_cells_alone(crafted_sets):
    gauss, rows, n = crafted_sets[0]
    for cols in (S.RADIANCE_COLS, S.TRANS_COLS):
        t0 = S.poison(S.random_table(n), S.written_cells(n, gauss, cols))
        got = S.ordered_reduce(gauss, rows, t0, cols)
        w = S.written_cells(n, gauss, cols)
        assert (S.bits(got)[~w] == S.bits(t0)[~w]).all()        # -0.0 and every NaN payload as they were
        assert np.isfinite(got[w]).all() and (S.bits(got)[w] != S.bits(t0)[w]).any()
        assert (~w).sum() >= n * 3 and (S.bits(t0)[~w] == 0x80000000).any() and np.isnan(t0[~w]).any()


def test_table_value_is_added_last(crafted_sets):
    """table <- table + a_0: the sum of the records is formed from +0 and the table's value joins once, at the end"""
    gauss, rows, n = crafted_sets[1]
    t0 = S.random_table(n)
    zero = np.zeros_like(t0)
    alone = S.ordered_reduce(gauss, rows, zero)
    both = S.ordered_reduce(gauss, rows, t0)
    w = S.written_cells(n, gauss, S.RADIANCE_COLS)
    assert (S.bits((t0 + alone).astype(np.float32))[w] == S.bits(both)[w]).all()


@pytest.mark.parametrize("variant", S.WRONG)
def test_a_wrong_order_changes_bits(crafted_sets, variant):
    changed = 0
    for gauss, rows, n in crafted_sets:
        t0 = S.random_table(n)
        ref, other = S.ordered_reduce(gauss, rows, t0), S.ordered_reduce(gauss, rows, t0, variant=variant)
        changed += int((S.bits(ref) != S.bits(other)).sum())
        one = [(j, lo, hi) for j, lo, hi in S.segments(gauss) if hi - lo == 1][0][0]
        if variant != "from_table":
            assert (S.bits(ref)[one] == S.bits(other)[one]).all()       # a segment of one record has one order
    assert changed >= 1, variant


def test_aimed_bundle_stays_under_the_cap(oracle):
    g0 = oracle.grid_scene(16)
    o, d = S.aimed_rays(g0)
    assert d.shape == (4096, 3)
    u = G.undecided(o, d, g0)
    assert u.sum() <= 0.05 * len(g0), int(u.sum())
    sc = S.aimed(oracle)
    assert len(sc.g) == len(g0) - u.sum()
    lens = np.array([len(l) for l in sc.lists()])
    assert lens.min() >= 1 and lens.max() <= S.RAY_PL                    # short rays under the default cull_eps ...
    assert min(len(l) for l in sc.lists(0.0, 1)) > S.RAY_PL             # ... and long ones with cull_eps = 0: both kernels record
    hits = np.bincount(np.concatenate(sc.lists()), minlength=len(sc.g))
    assert hits.max() == 4096 and ((hits > 0) & (hits < 4096)).any()     # segments of 64 rounds, and partial ones


@pytest.mark.parametrize("k", S.K_RAYS)
def test_k_rays_give_one_segment_of_k(oracle, k):
    sc = S.k_rays(oracle, k)
    assert len(sc.d) == k and all(list(l) == [1] for eps in G.EPS for l in sc.lists(eps, 1))
    assert S.record_count([len(l) for l in sc.lists()], True) == k


def test_record_count():
    assert S.record_count([0, 1, S.RAY_PL, S.RAY_PL + 1], True) == 1 + S.RAY_PL + 2 * (S.RAY_PL + 1)
    assert S.record_count([0, 1, S.RAY_PL, S.RAY_PL + 1], False) == 1 + S.RAY_PL + S.RAY_PL + 1
