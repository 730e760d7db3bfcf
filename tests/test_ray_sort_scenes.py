"""CPU checks of tests/ray_sort_scenes.py: the model of the sorted bundles says what the sort is for (fewer member tests on bundles whose
neighbours share nothing), and the cases of tests/test_gpu_ray_sort.py can see the ways an implementation can go wrong.  No GPU.
"""
import numpy as np
import pytest

import ray_sort_scenes as R

_cache = {}


def main(oracle, indexed=True, shuffled=False):
    """(Spheres, mid keys, the model's own stable order) of the main case, in the bundle's order or under the seeded shuffle."""
    key = (indexed, shuffled)
    if key not in _cache:
        g, o, d = R.main_case(oracle)
        if shuffled:
            o, d, _ = R.shuffled_rays(o, d)
        sp = R.Spheres(g, o, d, indexed)
        _cache[key] = (sp, sp.keys(), R.sort_order(sp.keys()))
    return _cache[key]


# ---- what the sort is for ----
def test_main_case_is_what_it_claims(oracle):
    sp, keys, order = main(oracle)
    assert sp.rays == R.MAIN_RAYS and sp.keep[1].shape[1] == 65 and len(sp.size) == 65 and sp.size[-1] == 1
    assert not (keys == R.NONE).any()                              # every ray is aimed at a Gaussian
    assert len(np.unique(keys)) >= 32                               # many classes of rays
    assert (keys[:-1] != keys[1:]).mean() > 0.9                     # ... and neighbours in the bundle share nothing
    assert R.order_faults(order, keys) == []
    assert not np.array_equal(order, np.arange(sp.rays))


@pytest.mark.parametrize("shuffled", [False, True], ids=["bundle-order", "seeded-shuffle"])
def test_sorted_waves_test_fewer_members(oracle, shuffled):
    sp, keys, order = main(oracle, shuffled=shuffled)
    unsorted_lo = sp.members_tested(np.arange(sp.rays), 0)
    sorted_hi = sp.members_tested(order, 2)
    print("shuffled" if shuffled else "bundle order", "unsorted >=", unsorted_lo, "sorted <=", sorted_hi, "ratio", sorted_hi / unsorted_lo)
    assert sp.members_tested(order, 0) <= sorted_hi
    assert sorted_hi < unsorted_lo
    if shuffled:
        # the condition tests/test_gpu_ray_sort.py reads from the device; ray_sort_scenes.MAIN_RAYS says why 4096 rays and not 1024
        assert 2 * sorted_hi <= unsorted_lo


def test_1024_and_2048_rays_do_not_reach_the_half(oracle):
    """Why the main case has 4096 rays: the smallest power of two at which the condition above holds."""
    for count in (1024, 2048):
        g, o, d = R.main_case(oracle, count)
        o, d, _ = R.shuffled_rays(o, d)
        sp = R.Spheres(g, o, d, True)
        assert 2 * sp.members_tested(R.sort_order(sp.keys()), 2) > sp.members_tested(np.arange(count), 0), count


def test_without_the_index_the_chunk_spheres_leave_nothing_to_sort(oracle):
    """The cloud is not laid out along a curve: nearly every chunk sphere is kept by every ray, the keys hardly differ and the sorted
    order buys nothing -- the bundle is still sorted, by the chunk keys, and the GPU tests compare its bits."""
    sp, keys, order = main(oracle, indexed=False)
    assert len(np.unique(keys)) <= 8 and sp.keep[0].mean() > 0.95
    assert sp.members_tested(order, 2) > 0.9 * sp.members_tested(np.arange(sp.rays), 0)


# ---- the key ----
def test_keys_lie_in_their_own_bracket_and_none_means_nothing_kept(oracle):
    for indexed in (True, False):
        sp, keys, _ = main(oracle, indexed)
        for which in (0, 1, 2):
            assert sp.bracket_ok(sp.keys(which)).all()
        assert not sp.bracket_ok(np.full(sp.rays, R.NONE, np.uint32)).any()      # every ray keeps something for certain
    keep = np.zeros((3, 70000), bool)
    keep[0, [3, 9]] = True
    keep[1, [65535, 69999]] = True                                                 # clamped, and still not the key of "nothing"
    assert list(R.keys_of(keep)) == [(3 << 16) | 9, 0xFFFFFFFF, R.NONE] and R.keys_of(keep)[1] == R.NONE


def test_a_ray_that_keeps_nothing_sorts_last(oracle):
    g, o, d = R.main_case(oracle, 130)
    d = d.copy()
    d[[5, 77]] = R.S.normalise([[1.0, 0.0, 0.1], [0.0, 1.0, -0.2]])               # past the cloud (the spheres are tested against the LINE)
    sp = R.Spheres(g, o, d, True)
    keys = sp.keys()
    order = R.sort_order(keys)
    assert list(np.flatnonzero(keys == R.NONE)) == [5, 77] and list(order[-2:]) == [5, 77]
    assert R.order_faults(order, keys) == []
    assert "a ray without a sphere is not last" in R.order_faults(np.roll(order, 1), keys)


# ---- wrong variants the cases must be able to see ----
def test_order_applied_to_the_outputs_instead_of_the_inputs_is_seen(oracle):
    sp, keys, order = main(oracle)
    values = np.arange(sp.rays) * 7 + 1                                # any per-ray result
    np.testing.assert_array_equal(R.shade(values, order), values)
    wrong = R.shade(values, order, at_ray=False)
    assert (wrong != values).mean() > 0.9
    for n in (65, 130):                                                # ... and on the small sizes of the GPU suite
        g, o, d = R.main_case(oracle, n)
        k = R.Spheres(g, o, d, True).keys()
        v = np.arange(n) + 1
        assert (R.shade(v, R.sort_order(k), at_ray=False) != v).any(), n


def test_an_unstable_tie_order_is_seen(oracle):
    sp, keys, order = main(oracle)
    assert len(np.unique(keys)) < sp.rays                              # there are ties
    wrong = R.sort_order(keys, stable=False)
    assert R.order_faults(wrong, keys) == ["ties out of ray order"]
    assert sp.members_tested(wrong, 2) <= sp.members_tested(np.arange(sp.rays), 0)   # it is still a good order: only the order check sees it
    for n in (65, 130):
        g, o, d = R.main_case(oracle, n)
        k = R.Spheres(g, o, d, True).keys()
        assert R.order_faults(R.sort_order(k, stable=False), k) == ["ties out of ray order"], n


def test_a_key_without_the_leaf_test_is_seen_and_one_without_the_group_test_cannot_be(oracle):
    """A key from the group test alone (every leaf of a kept group) leaves every ray's bracket.  A key from the leaf tests alone, without
    the ray's own group test, does not, on this or any finite scene: a group sphere bounds its leaf spheres, so a line that reaches a leaf
    reaches its group, and the own-group test changes a key only where float32 rounding decides -- inside the bracket by definition."""
    g, o, d = R.main_case(oracle)
    sp, _, _ = main(oracle)
    assert not sp.bracket_ok(R.Spheres(g, o, d, True, leaf_test=False).keys()).any()
    assert sp.bracket_ok(R.Spheres(g, o, d, True, group_test=False).keys()).all()


def test_a_dropped_last_wave_is_seen(oracle):
    for n in (65, 130):
        g, o, d = R.main_case(oracle, n)
        sp = R.Spheres(g, o, d, True)
        order = R.sort_order(sp.keys())
        v = np.arange(n) + 1
        out = R.shade(v, order, last_wave=False)
        assert (out == -1).sum() == n % 64 and sorted(np.flatnonzero(out == -1)) == sorted(order[n // 64 * 64:])
        assert sp.members_tested(order, 2, last_wave=False) < sp.members_tested(order, 0)


# ---- the capacity cases ----
@pytest.mark.parametrize("cap, n", R.WIDE)
def test_wide_cases_mix_both_kernels_where_the_scene_allows(oracle, cap, n):
    g, o, d = R.wide_case(oracle, cap, n)
    lo, hi = R.S.kept_range(o, d, g)
    long_rays, short_rays = int((lo > R.RAY_PL).sum()), int((hi <= R.RAY_PL).sum())
    print(cap, n, "long", long_rays, "short", short_rays)
    assert len(d) == 130 and long_rays + short_rays >= 128
    if n > R.RAY_PL:
        assert long_rays >= 60                                         # the queue is filled by a sorted short kernel
    if (cap, n) == (R.RAY_PL, R.RAY_PL + 1):
        assert short_rays >= 30                                        # ... whose waves mix short and long rays
    if n > R.RAY_LCAP:
        assert (lo > R.RAY_LCAP).sum() >= 30                           # the scratch slot
    for indexed in (True, False):
        sp = R.Spheres(g, o, d, indexed)
        assert not np.array_equal(R.sort_order(sp.keys()), np.arange(130)) or len(np.unique(sp.keys())) == 1
