"""The scenes of the list kernels' suite (tests/list_scenes.py, rendered by tests/test_gpu_lists.py) can see what they are for --
properties of the float64 model and of the oracle alone, checked on the CPU with the same clouds, frames and plans as the GPU test:
the model is sure of every cone decision of every frame, the generator took out at most 5 % of what it drew, every family shows
what it was built to show, the model agrees with block_scenes.plan where the two overlap, and each of ten wrong variants of the model
changes a number that the GPU test holds.
"""
import numpy as np
import pytest

import block_scenes as B
import list_scenes as S
from list_scenes import ACTIVE, DENSE, EMPTY, LIGHT, MARK


def frames_of(oracle, name):
    c = S.cloud(oracle, name)
    return c, [(fr, S.plan_frame(oracle, c, fr)) for fr in c.frames]


@pytest.mark.parametrize("name", S.ALL_CLOUDS)
def test_the_model_is_sure_and_the_cloud_is_whole(oracle, name):
    """unsure == 0 in every frame made of the cloud -- raster (light filing) and sparse (none) --, and the generator removed at most
    5 % of what it drew: a condition that keeps it from hollowing a scene out, not a measurement."""
    c, plans = frames_of(oracle, name)
    assert c.removed <= S.REMOVED_MAX * c.drawn, (name, c.removed, c.drawn)
    assert len(c.g) == c.drawn - c.removed
    for fr, p in plans:
        assert p.unsure == 0, (name, fr.name, p.unsure)
        q = S.plan_frame(oracle, c, fr, light=False)
        assert q.unsure == 0 and S.observables(q) == S.observables(p) and q.classes[LIGHT] == 0
        assert q.classes[ACTIVE] == p.classes[ACTIVE] + p.classes[LIGHT]


def test_the_grid_shows_every_class(oracle):
    c, plans = frames_of(oracle, "grid")
    fr, p = plans[0]
    assert fr.mode == "device" and p.fused and p.refine and (p.L.tiles_w, p.L.tiles_h, p.L.cells_x, p.L.cells_y) == (4, 4, 2, 2)
    assert all(p.classes[k] >= 1 for k in (EMPTY, LIGHT, ACTIVE, DENSE)), p.classes
    assert any(S.PCAP < cell.count != MARK for cell in p.cells) and p.marked == 0           # dense by its own list, not by a mark
    assert p.dense_exact
    mag = c.g["magnitude"]
    assert (mag == 0).sum() >= 3 and (mag < 0).sum() >= 3
    G = B.geometry(S.view_of(oracle, c, fr.view), fr.eps, rays=False)
    zero, negative = np.flatnonzero(mag == 0), np.flatnonzero(mag < 0)
    assert np.isneginf(G.cull_x[zero]).all() and not any(j in cell.kept for cell in p.cells if cell.count for j in zero)
    assert any(j in cell.kept for cell in p.cells if cell.count for j in negative)          # |sigma mag| counts, not its sign


def test_partial_cells_and_blocks(oracle):
    """Tiles whose size is no multiple of 32, 8 or 4 pixels, a truncated tile size, tile grids and tiles that are not square."""
    _, [(_, p)] = frames_of(oracle, "p136")
    assert (p.L.tile_w, p.L.tile_h, p.L.cells_x, p.L.cells_y, p.L.stride) == (68, 68, 3, 3, 136) and p.refine
    assert sorted({c.inside for c in p.cells}) == [1, 4, 16]                                 # 4 pixels of the third cell: one block column
    _, [(_, p)] = frames_of(oracle, "cube")
    assert (p.L.tile_w, p.L.tile_h, p.L.cells_x, p.L.cells_y, p.L.stride) == (40, 27, 2, 1, 200) and p.refine and p.L.tile_h * p.L.tiles_h < 136
    assert sorted({c.inside for c in p.cells}) == [4, 16]                                    # 27 rows: four block rows, the last of 3 pixels
    assert len(S.cell_pixels(p.L, 1)) == 8 * 27 and len(S.cell_pixels(p.L, 0)) == 32 * 27
    _, [(_, p)] = frames_of(oracle, "t96")
    assert (p.L.tiles_w, p.L.tiles_h, p.L.tile_w, p.L.tile_h, p.L.cpt) == (4, 3, 24, 21, 1) and p.refine
    assert {c.inside for c in p.cells} == {9}
    for name in ("p136", "cube", "t96"):
        _, [(_, p)] = frames_of(oracle, name)
        assert p.classes[LIGHT] and p.classes[ACTIVE] and len(p.cells_lit) > 4
        pix = np.concatenate([S.cell_pixels(p.L, c.key) for c in p.cells])
        assert len(np.unique(pix)) == len(pix) == p.L.tile_w * p.L.tile_h * p.L.n_tiles   # the cells partition what the tiles cover


def test_tcap_in_one_tile_of_several(oracle):
    """Fused: one tile beyond TCAP, every cell of it marked, dense and on the tile's list, its neighbours with lists of their own.
    The same cloud through the unfused kernel: lists beyond TCAP and no mark; as one tile: a list beyond ref_n, a negative slack."""
    c, plans = frames_of(oracle, "narrow")
    (_, fused), (_, pair), (_, one) = plans
    assert fused.fused and fused.L.cpt == 4
    over = [t for t, n in enumerate(fused.totals) if n > S.TCAP]
    assert len(over) == 1 and 1025 <= fused.totals[over[0]] <= 1400 and fused.marked == 4
    for cell in fused.cells:
        if cell.tile == over[0]:
            assert cell.count == MARK and cell.cls == DENSE and cell.n_list == fused.totals[over[0]]
        else:
            assert cell.count != MARK and cell.n_list == cell.count
    assert not pair.fused and pair.L.cpt == 81 and pair.L.n_tiles == 2 and pair.refine
    assert any(1025 <= n <= 1400 for n in pair.totals) and pair.marked == 0 and pair.classes[EMPTY] and pair.classes[ACTIVE] and pair.classes[DENSE]
    assert not one.fused and one.L.cpt == 72 and one.totals[0] > S.REF_N and one.slack_min < 0 and one.marked == 0


def test_caller_made_lists(oracle):
    c, plans = frames_of(oracle, "grid")
    by = {fr.mode: (fr, p) for fr, p in plans if not fr.chunks}
    assert S.observables(by["lists"][1]) == S.observables(by["device"][1]) and by["lists"][1].fused
    fr, minus = by["lists-minus"]
    t, victim = fr.victim
    assert victim in S.tile_lists(S.view_of(oracle, c, fr.view).ref)[t]                   # the device's tile test would keep it
    assert minus.totals[t] == by["lists"][1].totals[t] - 1 and minus.tile_entries < by["lists"][1].tile_entries
    assert not any(victim in cell.kept for cell in minus.cells if cell.tile == t)
    none = by["none"][1]
    assert none.L.n_tiles == 1 and none.L.cpt == 64 and none.fused and none.totals[0] <= S.TCAP
    assert none.cells_lit and S.observables(none) != S.observables(by["device"][1])          # another total, another slack


def test_no_refine(oracle):
    c, plans = frames_of(oracle, "norefine")
    (fr, dev), (_, host) = plans
    ref = S.tile_lists(S.view_of(oracle, c, fr.view).ref)
    assert (dev.L.tile_w, dev.L.stride, dev.L.n_tiles, dev.L.cpt) == (6, 96, 256, 1)
    assert not dev.refine and dev.fused and not host.refine and not host.fused
    for p in (dev, host):
        assert [cell.count for cell in p.cells] == [len(l) for l in ref] and p.unsure == 0
    assert dev.classes[LIGHT] and dev.classes[DENSE] and not host.classes[LIGHT]
    pix = np.concatenate([S.cell_pixels(dev.L, k) for k in range(256)])
    assert len(np.unique(pix)) == len(pix) == 96 * 96 and pix.max() == 96 * 96 - 1          # rows of 96 in an image of 100: the tiles drift


def test_thresholds(oracle):
    c, plans = frames_of(oracle, "grid-thresholds")
    by = {fr.name: (fr, p) for fr, p in plans}
    sc = S.view_of(oracle, c, S.GRID_VIEW)
    plain = S.plan_lists(sc)
    p7 = by["256x256-4x4-eps1e-07"][1]
    assert p7.tile_entries < plain.tile_entries
    G0, G0l = B.geometry(sc, 0.0, rays=False), B.geometry(sc, 0.0, floor=S.EXP_FLOOR["libm"], rays=False)
    live = c.g["magnitude"] != 0
    assert G0.floor[live].all() and (G0.cull_x[live] == S.EXP_FLOOR["vcl"]).all() and (G0l.cull_x[live] == 104.0).all()
    p0, p0l = by["256x256-4x4-eps0"][1], by["256x256-4x4-eps0-libm"][1]
    assert plain.tile_entries < p0.tile_entries < p0l.tile_entries
    # at the floor there is no slack: the same lists with and without it
    assert S.observables(S.plan_lists(sc, eps=0.0, ref_n=0.0)) == S.observables(p0)
    pr = by["256x256-4x4-ref_n0"][1]
    assert pr.slack_min == 0.0 and pr.tile_entries > plain.tile_entries
    many, [(fr, pm)] = frames_of(oracle, "many")
    Gm = B.geometry(S.view_of(oracle, many, fr.view), fr.eps, rays=False)
    assert 4096 < len(many.g) <= 8192 and Gm.eps_eff == pytest.approx(1e-9 * 4096 / len(many.g), rel=1e-6)
    assert all(n <= S.TCAP for n in pm.totals)


def test_two_orderings_one_model(oracle):
    """The chunk scenes: the same Gaussians shuffled and by raster rows.  The model knows nothing of order; the bounding spheres of 64
    consecutive Gaussians span the scene in the one and are tight in the other."""
    a, b = S.cloud(oracle, "grid"), S.cloud(oracle, "grid-rows")
    assert sorted(r.tobytes() for r in a.g) == sorted(r.tobytes() for r in b.g) and a.g.tobytes() != b.g.tobytes()
    pa, pb = S.plan_frame(oracle, a, a.frames[0]), S.plan_frame(oracle, b, b.frames[0])
    assert S.observables(pa) == S.observables(pb) and pa.totals == pb.totals

    def extent(g):
        mu = g["mu"][:len(g) // 64 * 64, :3].reshape(-1, 64, 3)
        return float(np.linalg.norm(mu.max(1) - mu.min(1), axis=1).mean())
    assert extent(b.g) < 0.75 * extent(a.g)


def test_two_cameras(oracle):
    c, [(_, pa), (_, pb)] = frames_of(oracle, "grid-cameras")
    assert S.observables(pa) != S.observables(pb) and pa.cells_lit != pb.cells_lit


@pytest.mark.parametrize("key", [("lane",), ("factors", "plain"), ("inst", 9, "last"), ("ragged", "both")], ids=lambda k: "-".join(map(str, k)))
def test_the_model_restates_the_block_suites_levels(oracle, key):
    """On a scene of one tile and one cell the tile and cell levels are those block_scenes.plan restates to count what enters a block."""
    sc = B.scene(oracle, key)
    view = B.Scene(sc, ref=oracle.tile_gaussians(sc.tw, sc.th, sc.g, sc.view))
    p = S.plan_lists(view, eps=B.EPS_TEST)
    want = B.plan(sc, B.EPS_TEST)
    assert p.L.n_tiles == 1 and p.L.cpt == 1 and p.unsure == 0
    assert p.tile_entries == want.tile_entries and p.shaded_blocks == want.n_blocks
    assert p.cells[0].n_list == want.blocks[0].n_list


@pytest.mark.parametrize("wrong", S.WRONG)
def test_the_scenes_can_see_the_mistake(oracle, wrong):
    """Each wrong variant of the model changes cells_lit, shaded_blocks or tile_entries of at least one frame the GPU suite renders."""
    seen = []
    for name in S.ALL_CLOUDS:
        c = S.cloud(oracle, name)
        for fr in c.frames:
            if S.observables(S.plan_frame(oracle, c, fr, wrong=wrong)) != S.observables(S.plan_frame(oracle, c, fr)):
                seen.append(f"{name}-{fr.name}")
    print(wrong, "shows in", seen)
    assert seen, wrong
