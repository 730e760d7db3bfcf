"""The scenes of the exact dense body's suite (tests/dense_scenes.py, rendered by tests/test_gpu_dense.py) can see what they are for
-- properties of the float64 model and of the reference alone, checked on the CPU with the same builders and pixels as the GPU
test: the tile holds the stack, a lost marker shows, the three classes of (chunk, absorber) visits all occur and the model is sure
of its counts, tied keys are tied in float32 too.
"""
import numpy as np
import pytest

import dense_scenes as D

SINGLE_BLOCK = [("stack", n) for n in D.LENGTHS] + [("ties", False), ("ties", True)]
ALL_SCENES = SINGLE_BLOCK + [("ragged", name) for name in D.RAGGED]
SHARE_MIN, BRACKET_MAX = 0.10, 0.01     # of a scene's visits: what each class takes at least, what the model may leave open
KEY_GAP = 1e-4                          # keys are 35 .. 66: an fp32 key is good to ~1e-5


def ident(key):
    return f"{key[0]}-{key[1]}"


def test_deal_ranks_by_hand():
    assert D.deal_ranks(25) == [0, 23, 24]                                  # one member in the last chunk; 23 | 24: the round of 4 waves
    assert D.deal_ranks(30) == [0, 23, 24, 25, 26, 27, 28, 29]              # a full last chunk
    assert D.deal_ranks(49) == [0, 23, 24, 47, 48]
    assert D.deal_ranks(97) == [0, 23, 24, 47, 48, 95, 96]
    assert D.deal_ranks(193) == [0, 23, 24, 47, 48, 95, 96, 192]
    assert D.chunks(7) == [[0, 1, 2, 3, 4, 5], [6, 6, 6, 6, 6, 6]] and D.chunks(6) == [[0, 1, 2, 3, 4, 5]]
    assert D.visit_total([7]) == 14 and D.visit_total([25, 97]) == 5 * 25 + 17 * 97


def test_plan_restates_the_body_by_hand(oracle):
    """Seven Gaussians on the axis, one unit apart (36 .. 42 from the camera), sigma 0.2 (r = 3.54), listed out of depth order: the
    first chunk holds depths 36 .. 41, the second depth 42 alone, padded with itself.  The rays' cosines (>= 0.9992) move nothing
    near a threshold.
      chunk 1, samples [36 - 0.8, 41]: its own six members are `full` (hi >= 0); the absorber at 42 has hi = (41 - 42) 3.54 = -3.54:
        behind every sample for Taylor (SAT 2), not for A&S (5.5).
      chunk 2, samples [42 - 0.8, 42]: lo = (41.2 - mubar_j) 3.54 = 18.4, 14.8, 11.3, 7.8, 4.2, 0.7, < 0 for the absorbers at 36 ..
        42: four in front of every sample for A&S, five for Taylor.
    Then the model against a restatement in plain loops."""
    z = np.array([3.0, 0.0, 6.0, 1.0, 5.0, 2.0, 4.0])
    mu = np.stack([np.zeros(7), np.zeros(7), z], 1)
    sc = D.bare(oracle, np.full((7, 4), 0.5), mu, np.full(7, 0.2), np.full(7, 0.1))
    assert sc.tiles["offsets"][1] == 7
    assert list(D.depth_order(sc)) == [1, 3, 5, 0, 6, 4, 2]
    p = D.plan(sc, D.SAT[D.ERF_AS])
    assert (p.total, p.zero, p.common, p.full) == (14, (0, 0), (4, 4), (10, 10))
    p = D.plan(sc, D.SAT[D.ERF_TAYLOR])
    assert (p.total, p.zero, p.common, p.full) == (14, (1, 1), (5, 5), (8, 8))
    # plain loops, the kernel's own order: chunk, absorber, ray
    G, order = D.geometry(sc), D.depth_order(sc)
    for sat in D.SAT.values():
        zero = common = 0
        for i0 in range(0, 7, 6):
            members = [order[i0 + e] if i0 + e < 7 else order[i0] for e in range(6)]
            for j in order:
                all_zero = all_common = True
                for ray in range(64):
                    s_max = max(G.mubar[ray, e] for e in members)
                    s_min = min(G.mubar[ray, e] - 4.0 * G.sigma[e] for e in members)
                    m = G.mubar[ray, j] * G.r[j]
                    hi, lo = s_max * G.r[j] - m, s_min * G.r[j] - m
                    all_zero &= m >= sat and hi <= -(sat + 1e-3)
                    all_common &= m >= sat and lo >= sat + 1e-3
                zero += all_zero
                common += (not all_zero) and all_common
        p = D.plan(sc, sat)
        assert p.zero[0] <= zero <= p.zero[1] and p.common[0] <= common <= p.common[1]
        assert p.zero[1] - p.zero[0] <= 1 and p.common[1] - p.common[0] <= 1


@pytest.mark.parametrize("key", ALL_SCENES, ids=ident)
def test_scene_holds_its_stack_and_shows_a_lost_marker(oracle, key):
    """The tile holds all n (every tile of the four); every block has a ray that keeps more than the block kernel's 24, which
    hands it to the dense path; leaving any one marker out moves a checked pixel by at least MARKER_FACTOR tolerances of the GPU test."""
    sc = D.scene(oracle, key)
    counts = np.diff(sc.tiles["offsets"])[:sc.tiles["w"] * sc.tiles["h"]]
    assert (counts == sc.n).all(), counts
    whole = D.blocks_go_dense(sc)
    assert key[0] == "ragged" or whole == 1                                 # ... and the one block's candidates are all n
    peak = float(sc.orad.max())
    tol = D.tolerance(sc.n, peak)
    assert tol == 1e-4                                                      # n > 24 and a peak below 1
    assert sc.orad[:, :3].max(1).min() > 0.01                               # no black pixel: L of the derived bounds is a radiance
    want = {int(sc.order[k]) for k in D.deal_ranks(sc.n)}
    assert want <= set(sc.markers) and len(sc.markers) == len(want) + (0 if key == ("ties", True) else len(sc.groups))
    effects, _ = D.marker_effects(oracle, sc)
    print(ident(key), f"n={sc.n} peak={peak:.3f} markers={len(sc.markers)} weakest marker {min(effects.values()) / tol:.1f} tolerances")
    for k, e in effects.items():
        assert e >= D.MARKER_FACTOR * tol, (k, e)


@pytest.mark.parametrize("key", SINGLE_BLOCK, ids=ident)
def test_every_class_of_visit_occurs_and_the_model_is_sure(oracle, key):
    """Keys that differ differ by far more than an fp32 key's error, so the kernel's depth order is the model's.  For the SAT of
    every Erf variant each of zero, common and full takes at least 10 % of the visits and the model leaves at most 1 % of them open
    -- a condition on the scenes.  Gaussians that all share one centre cannot saturate one another: there every visit is `full`,
    for certain."""
    sc = D.scene(oracle, key)
    k = np.sort(D.keys(sc, np.arange(64)))
    gaps = np.diff(k)
    assert (gaps[gaps > 0] >= KEY_GAP).all() if (gaps > 0).any() else key == ("ties", True)
    for erf, sat in D.SAT.items():
        p = D.plan(sc, sat)
        assert p.total == -(-sc.n // 6) * sc.n
        print(ident(key), D.ERF_NAMES[erf], f"visits {p.total} zero {p.zero} common {p.common} full {p.full}")
        if key == ("ties", True):
            assert p.zero == p.common == (0, 0)
            continue
        for lo, hi in (p.zero, p.common, p.full):
            assert lo >= SHARE_MIN * p.total, (erf, lo, p.total)
            assert hi - lo <= BRACKET_MAX * p.total, (erf, lo, hi, p.total)


@pytest.mark.parametrize("same_depth", [False, True])
def test_tied_keys_are_tied_in_float32(oracle, same_depth):
    """The members of a group have bit-equal keys as the kernel computes them (from centre - origin in fp32), other Gaussians do
    not share them; ties are ranked by list position; a group of seven spans two chunks."""
    sc = D.scene(oracle, ("ties", same_depth))
    k32 = D.keys32(sc, np.arange(64))
    assert [len(ids) for ids in sc.groups] == ([30] if same_depth else list(D.TIE_GROUPS))
    tied = np.zeros(sc.n, bool)
    for ids in sc.groups:
        assert len(set(k32[ids].tobytes()[4 * i:4 * i + 4] for i in range(len(ids)))) == 1
        assert (np.diff(ids) > 0).all()
        ranks = np.array([int(np.nonzero(sc.order == i)[0][0]) for i in ids])
        assert (np.diff(ranks) == 1).all()                                  # neighbours in depth, in list order
        plain = [i for i in ids if int(i) not in sc.markers]                # (the markers share four colours)
        assert len(set(sc.g["magnitude"][ids])) == len(ids) and len({tuple(a) for a in sc.g["albedo"][plain]}) == len(plain)
        if not same_depth:
            assert sum(int(i) in sc.markers for i in ids) >= 1
        tied[ids] = True
    assert len(set(k32[~tied])) == (~tied).sum() and not set(k32[~tied]) & set(k32[tied])
    assert max(len(ids) for ids in sc.groups) > D.EC


def test_ragged_geometries_cut_blocks(oracle):
    """20x12 as one tile: six blocks, the right column four pixels wide, the bottom row four high; 20x20 as four tiles of 10x10: four
    blocks per tile of 64, 16, 16 and 4 pixels.  Every pixel belongs to exactly one block's writing lanes."""
    for name, blocks, sizes in (("one-tile-20x12", 6, [64, 64, 32, 32, 32, 16]), ("four-tiles-20x20", 16, [64, 16, 16, 4] * 4)):
        sc = D.scene(oracle, ("ragged", name))
        bl = D.blocks_of(sc)
        assert len(bl) == blocks and [int(v.sum()) for _, v in bl] == sizes
        written = np.concatenate([pix[v] for pix, v in bl])
        assert sorted(written) == list(range(sc.w * sc.h))
