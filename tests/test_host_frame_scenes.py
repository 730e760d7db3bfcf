"""The scenes of the host-frame delivery suite (tests/host_frame_scenes.py, run on the device by tests/test_gpu_host_frame_cells.py) can
see what they are for, checked on the CPU: every geometry is the hand-worked one, every crafted scene lights exactly the cells it
names by the list suite's cull model (tests/list_scenes.py) with room to spare, the delivery model writes what the rules say on three
hand-worked sequences, and each wrong variant of the model changes a mode or a written set of at least one case.
"""
import numpy as np
import pytest

import host_frame_scenes as H
import list_scenes as L
from block_scenes import Scene

# n_cells, refine, fused, and per geometry some cells worked by hand: key -> (first word, last word, number of words)
BY_HAND = {
    "128x128": (16, True, True, {0: (0, 31 * 128 + 31, 1024), 6: (32 * 128 + 64, 63 * 128 + 95, 1024), 15: (96 * 128 + 96, 127 * 128 + 127, 1024)}),
    "96x40": (6, True, True, {1: (32 * 96, 39 * 96 + 31, 8 * 32), 4: (64, 31 * 96 + 95, 1024), 5: (32 * 96 + 64, 39 * 96 + 95, 8 * 32)}),
    "32x32": (1, True, True, {0: (0, 1023, 1024)}),
    "64x32": (2, True, True, {1: (32, 31 * 64 + 63, 1024)}),
    "70x44": (8, True, True, {1: (32, 21 * 70 + 34, 3 * 22), 2: (35, 21 * 70 + 66, 32 * 22), 7: (22 * 70 + 67, 43 * 70 + 69, 3 * 22)}),
    "80x54": (8, True, True, {1: (32, 26 * 80 + 39, 8 * 27), 6: (27 * 80 + 40, 53 * 80 + 71, 32 * 27)}),
    "65x33": (4, False, True, {0: (0, 15 * 64 + 31, 512), 3: (16 * 64 + 32, 31 * 64 + 63, 512)}),
    "288x288": (81, True, False, {80: (256 * 288 + 256, 287 * 288 + 287, 1024)}),
    "96x96": (16, True, True, {3: (32 * 96 + 32, 47 * 96 + 47, 256), 13: (48 * 96 + 80, 79 * 96 + 95, 16 * 32)}),
    "128x128/4": (16, True, True, {5: (32 * 128 + 32, 63 * 128 + 63, 1024)}),
    "64x32/3": (6, True, True, {4: (24 * 64, 31 * 64 + 31, 8 * 32), 5: (24 * 64 + 32, 31 * 64 + 63, 8 * 32), 2: (12 * 64, 23 * 64 + 31, 12 * 32)}),
}


def deliveries(case, wrong=None):
    return [(i, s, e) for i, (s, e) in enumerate(zip(case.steps, H.run(case, wrong))) if e is not None]


@pytest.mark.parametrize("name", list(H.GEOMETRIES))
def test_every_geometry_is_the_hand_worked_one(name):
    (w, h, _, _), want = H.GEOMETRIES[name]
    g = H.geometry(name)
    assert (g.tiles_w, g.tiles_h, g.tile_w, g.tile_h, g.stride, g.cells_x, g.cells_y) == want
    n_cells, refine, fused, cells = BY_HAND[name]
    assert (g.n_cells, g.refine, g.fused, g.npix, g.pixels) == (n_cells, refine, fused, w * h, w * h)
    for key, (first, last, n) in cells.items():
        px = H.cell_pixels(g, key)
        assert (int(px[0]), int(px[-1]), len(px)) == (first, last, n), (name, key)
    # the cells are disjoint and cover what the tiles cover of the image
    mine = np.concatenate([H.cell_pixels(g, k) for k in range(g.n_cells)])
    covered = min(g.npix, g.stride * g.tile_h * g.tiles_h)
    np.testing.assert_array_equal(np.sort(mine), np.arange(covered))
    owner = H.cell_of_word(H.geometry(name, pixels=g.npix + 7))
    assert (owner[g.npix:] == -2).all() and (owner[covered:g.npix] == -1).all() and (owner[:covered] >= 0).all()


def test_the_geometries_show_what_they_are_for():
    g = {name: H.geometry(name) for name in H.GEOMETRIES}
    assert (g["96x40"].n_cells + 3) // 4 == 2 and g["96x40"].n_cells % 4 == 2                     # a last workgroup of two waves
    a = g["70x44"]                                                                               # dwords by the tile width
    assert a.tile_w % 4 == 3 and a.npix % 4 == 0 and 32 < a.tile_w < 36                          # the quad at column 32 straddles the tile's edge
    assert len(H.cell_pixels(a, 1, "columns-beyond-tile")) == 4 * 22
    b = g["80x54"]                                                                               # quads, a partial cell of two quads a row
    assert b.tile_w % 4 == 0 and b.npix % 4 == 0 and b.tile_w - 32 == 8 and b.tile_h < 32
    c = g["65x33"]                                                                               # dwords by the pixel count
    assert c.tile_w % 4 == 0 and c.npix % 4 == 1 and c.stride < c.w and c.npix - c.stride * c.tile_h * c.tiles_h == 97
    assert g["288x288"].cpt > H.MAX_FUSED_CELLS and not H.keeps_stamps(g["288x288"]) and not H.keeps_stamps(g["128x128"], retain=False)
    d = g["64x32/3"]                                                                             # `pix < npix` decides
    assert d.stride == d.w and d.tile_h * d.tiles_h == 36 > d.h
    assert len(H.cell_pixels(H.geometry("64x32/3", pixels=64 * 36), 4, "beyond-image")) == 12 * 32
    assert len({H.geometry(n, bg).sig for n in ("128x128", "96x96", "128x128/4") for bg in H.BG}) == 6      # every fall-back is another signature
    assert all(H.POISON not in (0, bg) for bg in H.BG.values())


# ---- the scenes light what they name ----
def crafted():
    """Every (geometry, scene) that a case delivers, renders or frames."""
    seen = {}
    for case in H.CASES.values():
        for s in case.steps:
            if s.op in ("deliver", "frame", "render"):
                geo = H.geometry(s.geo)
                seen[(s.geo, H.scene_of(geo, s.what).what)] = geo
    return seen


def lit_by_the_cull_model(oracle, geo, g):
    cam, _ = oracle.cli_camera(geo.w, geo.h)
    view = oracle.camera_view(cam)
    origin = np.array(cam.position[:], np.float32)
    np.testing.assert_array_equal(origin, H.EYE.astype(np.float32))
    plane = oracle.camera_plane(cam)
    # the camera that host_frame_scenes places its Gaussians under is this one
    x, y = geo.w - 1, geo.h - 1
    np.testing.assert_allclose([plane[0][-1], plane[1][-1], plane[2][-1]], H.at_pixel(geo, x, y, depth=1.0), atol=1e-6)
    sc = Scene(g=g, n=len(g), w=geo.w, h=geo.h, tw=geo.tw, th=geo.th, plane=plane, view=view, origin=origin,
               ref=oracle.tile_gaussians(geo.tw, geo.th, g, view))
    p = L.plan_lists(sc)
    assert (p.L.tiles_w, p.L.tiles_h, p.L.tile_w, p.L.tile_h, p.L.cpt) == (geo.tiles_w, geo.tiles_h, geo.tile_w, geo.tile_h, geo.cpt)
    assert p.fused == geo.fused and p.refine == geo.refine
    return p


def test_spots_light_the_cells_they_name_and_no_neighbour(oracle):
    """By the project's cull bound (list_scenes.plan_lists: the reference's tile test, the tile and cell cones, the cell slack), with
    no decision inside the model's margin; and the same at 1.5 times the spots' sigma -- the cull radius grows with it in proportion --
    so that every dark neighbour is dark with room to spare."""
    scenes = crafted()
    assert len(scenes) > 60
    for (name, what), geo in scenes.items():
        sc = H.scene_of(geo, what)
        fat = [1.0] if isinstance(what, str) else [1.0, 1.5]
        for f in fat:
            g = sc.g if f == 1.0 else H.spots(geo, what, fatten=f)
            p = lit_by_the_cull_model(oracle, geo, g)
            assert p.unsure == 0 and p.cells_lit == set(sc.lit), (name, what, f, sorted(p.cells_lit))
        if what == "flood":
            assert len(sc.lit) == geo.n_cells
    k12, k13 = H.scene_of(H.geometry(H.BASE), H.K12), H.scene_of(H.geometry(H.BASE), H.K13)
    assert 4 * len(k12.lit) == 3 * 16 and 4 * len(k13.lit) > 3 * 16                            # either side of the 3/4 edge


# ---- the model on hand-worked sequences ----
def rect(w, x0, y0, nx, ny):
    return np.sort(((x0 + np.arange(nx))[None, :] + w * (y0 + np.arange(ny))[:, None]).ravel())


def test_model_light_move_dark_by_hand():
    geo = H.geometry("128x128")
    m = H.DeliveryModel()
    m.register("A", geo.pixels)
    mode, written = m.deliver("A", geo, {1, 6}, True)
    assert mode == "full" and np.array_equal(written, np.arange(128 * 128))
    # cell 1: tile 0, cell 1 = columns 32 .. 63 of rows 0 .. 31; cell 6: tile 1 (right), cell 2 = columns 64 .. 95 of rows 32 .. 63;
    # cell 12: tile 3 (below right), cell 0 = columns 64 .. 95 of rows 64 .. 95
    c1, c6, c12 = rect(128, 32, 0, 32, 32), rect(128, 64, 32, 32, 32), rect(128, 64, 64, 32, 32)
    mode, written = m.deliver("A", geo, {6, 12}, True)
    assert mode == "delta" and np.array_equal(written, np.sort(np.concatenate([c1, c6, c12])))       # 1 reset, 6 again, 12 new
    mode, written = m.deliver("A", geo, set(), True)
    assert mode == "delta" and np.array_equal(written, np.sort(np.concatenate([c6, c12])))
    mode, written = m.deliver("A", geo, set(), True)
    assert mode == "delta" and len(written) == 0
    mode, written = m.deliver("A", H.geometry("128x128", "opaque"), set(), True)                     # another background
    assert mode == "full" and len(written) == 128 * 128
    mode, written = m.deliver("A", geo, {1}, False)                                                  # no stamps
    assert mode == "full"
    mode, written = m.deliver("A", geo, {1}, True)                                                   # ... and nothing recorded
    assert mode == "full"
    mode, written = m.deliver("A", geo, {1}, True)
    assert mode == "delta" and np.array_equal(written, c1)


def test_model_dense_switch_by_hand():
    """16 cells: 13 switch, 12 do not; the count a delivery reads is that of the launch before the previous launch."""
    geo = H.geometry("128x128")
    for k, modes, reads in ((12, "fddddd", [0, 0, 12, 12, 12, 12]), (13, "fdffff", [0, 0, 13, 13, 13, 13])):
        m = H.DeliveryModel()
        m.register("A", geo.pixels)
        got, seen = "", []
        for _ in range(6):
            seen.append(m.published("A"))
            got += m.deliver("A", geo, set(range(k)), True)[0][0]
        assert (got, seen) == (modes, reads), k
    # in: 2, 3, 3 cells counted, then floods of 16 -- the third flood is the first full one; out: two sparse frames are still full
    m = H.DeliveryModel()
    m.register("A", geo.pixels)
    seq = [{1, 6}, {1, 7}, {2, 7}] + [set(range(16))] * 4 + [{2, 7}, {2, 8}, {3, 8}]
    seen, got = [], ""
    for lit in seq:
        seen.append(m.published("A"))
        got += m.deliver("A", geo, lit, True)[0][0]
    assert seen == [0, 0, 2, 3, 3, 16, 16, 16, 16, 2] and got == "fddddffffd"
    # a delivery without stamps launches nothing: the two words keep their turn
    m = H.DeliveryModel()
    m.register("A", geo.pixels)
    for lit, stamps, want in ((set(range(16)), True, 0), (set(range(16)), True, 0), (set(range(16)), False, 16), ({1}, True, 16), ({1}, True, 16), ({1}, True, 1)):
        assert m.published("A") == want
        m.deliver("A", geo, lit, stamps)


def test_model_buffers_by_hand():
    geo = H.geometry("128x128")
    c1, c2, c3 = rect(128, 32, 0, 32, 32), rect(128, 0, 32, 32, 32), rect(128, 32, 32, 32, 32)
    m = H.DeliveryModel()
    for b in ("A", "B", "C"):
        m.register(b, geo.pixels)
    assert [m.bufs[b].slot for b in "ABC"] == [0, 1, 2]
    assert m.deliver("A", geo, {1}, True)[0] == m.deliver("B", geo, {2}, True)[0] == "full"
    mode, written = m.deliver("A", geo, {1}, True)                                   # B's frame in between is not A's history
    assert mode == "delta" and np.array_equal(written, c1)
    for _ in range(3):
        m.deliver("B", geo, set(range(16)), True)
    assert m.published("B") == 16
    m.unregister("B")
    m.register("B", geo.pixels)                                                      # the lowest free slot, its words cleared
    assert m.bufs["B"].slot == 1 and m.published("B") == 0 and m.slots[1].tally == [0, 0]
    assert m.deliver("B", geo, {3}, True)[0] == "full"
    mode, written = m.deliver("B", geo, {2}, True)
    assert mode == "delta" and np.array_equal(written, np.sort(np.concatenate([c2, c3])))
    mode, written = m.deliver("A", geo, {2}, True)                                   # A's history is still its own
    assert mode == "delta" and np.array_equal(written, np.sort(np.concatenate([c1, c2])))
    for i in range(13):
        m.register(f"X{i}", geo.pixels)
    with pytest.raises(H.Refused):
        m.register("one too many", geo.pixels)
    big = H.geometry("96x96", pixels=128 * 128)                                      # a larger buffer: the full copy ends at w * h
    m.unregister("X0")
    m.register("L", big.pixels)
    mode, written = m.deliver("L", big, {0}, True)
    assert mode == "full" and np.array_equal(written, np.arange(96 * 96))


# ---- the cases ----
def test_the_cases_cover_the_modes_they_are_for():
    modes = {name: "".join(e.mode[0] for _, _, e in deliveries(case)) for name, case in H.CASES.items()}
    for name in ("81-cells", "no-retain"):
        assert set(modes[name]) == {"f"}, name
    assert modes["repeated-pose"] == "fddddd"
    assert modes["fall-backs"] == "fd" * 7
    assert modes["dense-12"] == "fddddd" and modes["dense-13"] == "fdffff"
    assert modes["dense-lag"] == "fddddffffdd"
    assert modes["dense-union"] == "fddffdd"                     # |lit| = 8, |lit u held| = 16
    assert modes["dense-no-stamps"] == "fdffffdd"
    case = H.CASES["sixteen-buffers"]
    assert sum(s.op == "register" and s.refused for s in case.steps) == 1
    again = [i for i, s in enumerate(case.steps) if s.op == "register" and s.buf == "B08"][1]
    after = [(s.buf, e.mode) for i, s, e in deliveries(case) if i > again]
    assert [m for b, m in after if b == "B08"] == ["full", "delta", "full", "full"]            # the tally starts at zero: the lag of two deliveries again
    assert [m for b, m in after if b == "B07"] == ["delta"] * 4 and [m for b, m in after if b == "B10"] == ["full"] * 4
    # every delta of the case list writes less than the frame somewhere, and some delta leaves a cell alone that is dark and was dark
    assert any(e.mode == "delta" and len(e.written) == 0 for case in H.CASES.values() for _, _, e in deliveries(case))
    # a larger buffer keeps words beyond w * h that no delivery writes
    for name in ("larger-buffer", "overhang", "dense-no-stamps", "fall-backs"):
        assert any(e.geo.pixels > e.geo.npix and (len(e.written) == 0 or e.written[-1] < e.geo.npix) for _, _, e in deliveries(H.CASES[name]))
    assert H.UNSYNCED in H.CASES and len(H.CASES[H.UNSYNCED].buffers) == 2


def test_every_wrong_variant_is_seen_by_a_case(capsys):
    right = {name: deliveries(case) for name, case in H.CASES.items()}
    lines = []
    for wrong in H.WRONG:
        seen = []
        for name, case in H.CASES.items():
            for (i, _, a), (_, _, b) in zip(right[name], deliveries(case, wrong)):
                if a.mode != b.mode or not np.array_equal(a.written, b.written):
                    seen.append(f"{name}[{i}]")
                    break
        lines.append(f"{wrong:24s} {' '.join(seen) or '-- unseen --'}")
        assert seen, f"no case sees the variant {wrong}"
    with capsys.disabled():
        print("\nwrong variant            first step of each case that sees it")
        print("\n".join(lines))
