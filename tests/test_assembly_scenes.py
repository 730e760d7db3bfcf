"""The scenes of the frame assembly suite (tests/assembly_scenes.py, run on the device by tests/test_gpu_assembly.py) can see what they
are for -- properties of the numpy model alone, checked on the CPU with the same geometries, crafted frames, retained sequences and
buffer rotations as the GPU test: every geometry is the one its name promises, the model agrees with sharding.py where the tiles divide
the image and is a bijection of the covered span where they do not, the retained model equals the full assembly at every step, no
sentinel reaches an expected image, and each wrong variant of the model changes an image that the GPU test holds.
"""
import numpy as np
import pytest

import assembly_scenes as S
from assembly_scenes import BG, CELL, HDR, sharding

FULL_CASES = [(name, world) for name in S.GEOMETRIES for world in S.WORLDS] + [("32x32", 64)]


@pytest.mark.parametrize("name", list(S.GEOMETRIES))
def test_every_case_has_the_geometry_of_its_name(name):
    (w, h, _, _), want = S.GEOMETRIES[name]
    g = S.geo_of(name, 1)
    assert (g.tiles_w, g.tiles_h, g.tile_w, g.tile_h, g.stride) == want
    assert (g.w, g.h, g.npix) == (w, h, w * h) and g.covered == min(w * h, g.span)
    for world in S.WORLDS + (64,):
        q = S.geo_of(name, world)
        assert q.max_cells == q.slots * q.cpt and q.frame_cells == q.tiles * q.cpt and q.words == q.P + 1024 * q.max_cells and q.P % 4 == 0
        assert sorted(k for r in range(world) for k in S.owned(q, r)) == list(range(q.frame_cells))      # every cell has one owner


def test_the_geometries_show_what_they_are_for():
    g = {name: S.geo_of(name, 1) for name in S.GEOMETRIES}
    assert g["128x128"].frame_cells == 16 and (g["128x128"].tile_w % CELL, g["128x128"].tile_h % CELL) == (0, 0)
    a = g["71x45"]
    assert a.stride < a.w and a.tile_w % 4 == 3 and (a.cells_x, a.cells_y) == (2, 1) and a.npix - a.covered == 115
    # the last quad of the second cell column starts inside the tile and ends outside it
    quad = (a.tile_w - CELL) // 4 * 4 + CELL
    assert quad < a.tile_w < quad + 4
    pix, inside = S.cell_pixels(a, 1)
    assert inside[:a.tile_h, :3].all() and not inside[:, 3:].any() and not inside[a.tile_h:].any()
    assert (g["200x136"].npix - g["200x136"].covered, g["200x136"].cells_x, g["200x136"].cells_y) == (200, 2, 1)
    b = g["100x64"]
    assert b.stride > b.w and b.span == 6720 > b.npix == b.covered == 6400
    assert any(not S.cell_pixels(b, k)[1][:b.tile_h, :b.tile_w].all() for k in range(b.frame_cells))      # `pix < npix` decides somewhere
    c = g["96x40"]
    assert (c.cells_x, c.cells_y, c.tile_h - CELL) == (1, 2, 8) and c.tiles_w != c.tiles_h and c.tile_w != c.tile_h
    d = g["396x396"]
    assert d.frame_cells == 324 and d.frame_cells - 256 - 64 == 4                                      # second block, second wave: 4 lanes
    assert g["512x512"].tile_w * g["512x512"].tile_h == 4 * 64 * 256                                    # four passes of assemble_kernel's loop
    assert g["32x32"].frame_cells == 1 and g["64x32"].frame_cells == 2
    # world 8 over 2 x 2 tiles: ranks without a tile; world 3: padded slots beside owned ones
    assert sorted((S.geo_of("128x128", 8).table >= 0).sum(axis=1)) == [0, 0, 0, 0, 1, 1, 1, 1]
    t3 = S.geo_of("128x128", 3).table
    assert t3.shape == (3, 2) and sorted((t3 >= 0).sum(axis=1)) == [1, 1, 2]
    z = S.geometry(4, 4, 0.25, 0.25, 1)                                                                 # the geometry the calls must reject
    assert (z.tile_w, z.tile_h) == (0, 0)


@pytest.mark.parametrize("name", list(S.GEOMETRIES))
def test_the_linear_rule_is_a_bijection_of_the_span(name):
    """pix = tx*tile_w + x + stride*(ty*tile_h + y) maps (tile, x, y) one to one onto [0, span): where the tile size is truncated no
    raster mirror applies, and this is what stands in for it.  The cells' pixels are the same map, cut at the image's end."""
    g = S.geo_of(name, 1)
    t, y, x = np.meshgrid(np.arange(g.tiles), np.arange(g.tile_h), np.arange(g.tile_w), indexing="ij")
    pix = (t % g.tiles_w) * g.tile_w + x + g.stride * ((t // g.tiles_w) * g.tile_h + y)
    np.testing.assert_array_equal(np.sort(pix.ravel()), np.arange(g.span))
    mine = np.concatenate([p[i] for p, i in (S.cell_pixels(g, k) for k in range(g.frame_cells))])
    np.testing.assert_array_equal(np.sort(mine), np.arange(g.covered))


@pytest.mark.parametrize("name,world", [(n, w) for n in ("128x128", "96x40", "396x396", "512x512", "32x32", "64x32") for w in (1, 3, 8)])
def test_the_model_agrees_with_the_host_mirror_where_the_tiles_divide_the_image(name, world):
    g = S.geo_of(name, world)
    assert g.tile_w * g.tiles_w == g.w and g.tile_h * g.tiles_h == g.h
    rng = np.random.default_rng(9)
    for bg in BG.values():
        image = rng.integers(1, 1 << 24, (g.h, g.w)).astype(np.uint32) | np.uint32(S.PIXEL_TAG)
        for key in rng.choice(g.frame_cells, g.frame_cells // 2, replace=False):                        # half the cells are background
            pix, inside = S.cell_pixels(g, int(key))
            image.reshape(-1)[pix[inside]] = bg
        shards = [sharding.extract_sparse(image, g.table, r, g.tiles_w, g.tile_w, g.tile_h, background=bg) for r in range(world)]
        assert all(int(s[1]) == g.max_cells and int(s[2]) == g.cpt and len(s) == g.words for s in shards)
        mirror = sharding.scatter_sparse(shards, g.tiles_w, g.tile_w, g.tile_h, g.h, g.w, background=bg)
        np.testing.assert_array_equal(mirror, image)
        np.testing.assert_array_equal(S.full(shards, g, bg).reshape(g.h, g.w), image)


@pytest.mark.parametrize("name,world", FULL_CASES)
def test_crafted_frames_do_something_and_hold_no_sentinel(name, world):
    g = S.geo_of(name, world)
    for kind in S.KINDS if world <= 8 else ("half",):
        shards = S.frame_shards(g, kind, seed=7)
        assert len(shards) <= S.MAX_SHARDS and all(len(s) == g.words and s.dtype == np.uint32 for s in shards)
        for r, sh in enumerate(shards[:world]):
            n = int(sh[0])
            if kind == "half":                                                 # every free key and pixel slot holds the sentinel
                assert (n >= 1) == bool(S.owned(g, r)) and (sh[HDR + n:g.P] == S.SENT_FREE).all() and (sh[g.P + n * 1024:] == S.SENT_FREE).all()
            if kind == "stale-slots" and n < g.max_cells and sum(len(S.half(g, q, 7)) for q in range(world)) < g.frame_cells:   # valid keys behind n
                assert r > 0 or any(int(k) < g.frame_cells for k in sh[HDR + n:HDR + g.max_cells])
        for bg in BG.values():
            img = S.full(shards, g, bg)
            assert not S.has_sentinel(img)
            assert (img[g.covered:] == 0).all()
            lit = (img[:g.covered] != bg).sum()
            owners = sum(bool(S.owned(g, r)) for r in range(world))
            assert lit > 0 or (kind == "empty-shard" and owners == 1) or (kind == "beyond-grid" and g.max_cells <= 2 and owners == 1)
            assert not np.isin(img, [S.PREFILL]).any()
    if world <= 8:
        cap = g.max_cells
        assert int(S.frame_shards(g, "full", 7)[0][0]) == cap or world > 1
        assert any(int(s[0]) == cap + 5 for s in S.frame_shards(g, "overfull", 7))
        assert any(int(s[1]) == cap + 1 for s in S.frame_shards(g, "cap-off", 7)) and any(int(s[2]) == g.cpt + 1 for s in S.frame_shards(g, "cpt-off", 7))
        assert any(int(k) // g.cpt >= g.tiles for s in S.frame_shards(g, "beyond-grid", 7) for k in s[HDR:HDR + int(s[0])])


def test_two_shards_never_store_one_cell_with_different_pixels():
    for name, world in FULL_CASES:
        g = S.geo_of(name, world)
        for kind in S.KINDS if world <= 8 else ("half",):
            seen = {}
            for sh in S.frame_shards(g, kind, seed=7):
                for slot in range(min(int(sh[0]), g.max_cells)):
                    key, px = int(sh[HDR + slot]), sh[g.P + slot * 1024: g.P + (slot + 1) * 1024]
                    assert np.array_equal(seen.setdefault(key, px), px), (name, world, kind, key)
            if kind == "twice":
                assert sum(int(sh[0]) for sh in S.frame_shards(g, kind, 7)) > len(seen)


@pytest.mark.parametrize("name,world", S.SEQUENCES)
def test_the_retained_model_equals_the_full_assembly_at_every_step(name, world):
    """The public promise, for the single call and for the batch call with two buffers that swap places; and every sequence has steps
    where cells go dark, steps where none does and a step where all do."""
    steps = S.sequence(name, world)
    H, before, dark = S.Histories(), set(), []
    for st in steps:
        img = H.assemble("x", st.shards, st.geo, BG[st.bg], st.retained)
        want = S.expected(st)
        np.testing.assert_array_equal(img, want, err_msg=st.label)
        assert not S.has_sentinel(want)
        now = S.lit_keys(st)
        dark.append((len(before - now), len(before)))
        before = now
    assert any(d == 0 and n > 0 for d, n in dark) and any(0 < d < n for d, n in dark) and any(d == n > 0 for d, n in dark)
    labels = [st.label for st in steps]
    assert {"a header stops matching", "background changes", "plain assembly", "retained after plain", "one wave"} <= set(labels)
    assert ("last block" in labels) == (name == "396x396") and ("another grid" in labels) == (name == "128x128")
    stop = steps[labels.index("a header stops matching")]
    assert S.lit_keys(stop) < S.lit_keys(steps[labels.index("other half")])
    H = S.Histories()
    for call in S.alternating(name, world):
        (b0, s0), (b1, s1) = call
        got = H.assemble_batch([b0, b1], [s0.shards, s1.shards], s0.geo, BG[s0.bg], s0.retained)
        np.testing.assert_array_equal(got[0], S.expected(s0), err_msg=s0.label)
        np.testing.assert_array_equal(got[1], S.expected(s1), err_msg=s1.label)


@pytest.mark.parametrize("name", ["32x32", "64x32"])
def test_more_buffers_than_histories(name):
    """The rotation of the histories test in the model: which histories are dropped, and the full assembly throughout."""
    g = S.geo_of(name, 1)
    H = S.Histories()
    marks = {}
    for batch, bufs, rnd in S.history_ops():
        frames = [S.history_frame(g, S.buffer_number(b), rnd) for b in bufs]
        got = H.assemble_batch(bufs, frames, g, 0) if batch else [H.assemble(bufs[0], frames[0], g, 0)]
        for img, fr in zip(got, frames):
            np.testing.assert_array_equal(img, S.full(fr, g, 0), err_msg=f"{bufs} round {rnd}")
        marks[rnd] = len(H.evicted)
        assert len(H.h) <= S.MAX_FRAMES
    ev = H.evicted
    assert marks[1] == 0 and ev[:2] == ["A0", "A1"] and marks[3] == 2                       # the 65th buffer, then A0 again
    fourth = ev[marks[3]:marks[4]]
    assert len(fourth) == 64 and not any(b.startswith("B") for b in fourth)                 # the batch of B drops every A (and C), no B
    fifth = ev[marks[4]:marks[5]]
    assert sorted(fifth) == sorted(f"B{i}" for i in range(32, 64))                          # never a buffer of the batch itself
    assert marks[6] == marks[5]
    lit = [bool((S.full(S.history_frame(g, 0, rnd), g, 0) != 0).any()) for rnd in range(7)]
    assert True in lit and (False in lit or g.frame_cells > 1)


def test_batch_strides_stay_inside_the_contract():
    """A prefix never holds fewer cells than n except by one, and a stride of the header alone only travels with empty shards."""
    for name, world, F in S.BATCH_CASES:
        g = S.geo_of(name, world)
        frames = S.batch_frames(g, F, seed=11)
        names = []
        for label, stride, slots, fr in S.batch_strides(g, frames):
            names.append(label)
            k = max(S.fullest(f) for f in fr)
            assert stride % 4 == 0 and g.P <= stride <= g.words
            held = (stride - g.P) // 1024
            if label == "header":
                assert stride == g.P and k == 0
            elif label == "one-short":
                assert held == slots == k - 1 >= 1
                assert any((S.full(f, g, 0, slots) != S.full(f, g, 0)).any() for f in fr)           # the dropped slot shows
            else:
                assert held >= k and slots is None
        assert ("one-short" in names) == (name != "32x32")


def differs(a, b):
    return bool((a != b).any())


def test_each_wrong_variant_changes_an_image_the_gpu_test_holds():
    """variant -> the case of tests/test_gpu_assembly.py that sees it.  A variant that changed nothing would mean a hole in the cases."""
    used = set()

    def frame(name, world, kind, bg, wrong, slots=None):
        used.add(wrong)
        g = S.geo_of(name, world)
        sh = S.frame_shards(g, kind, seed=7)
        return differs(S.full(sh, g, BG[bg], slots, wrong), S.full(sh, g, BG[bg], slots))

    def one_short(name, world, wrong):
        used.add(wrong)
        g = S.geo_of(name, world)
        frames = S.batch_frames(g, 3, seed=11)
        slots = max(S.fullest(f) for f in frames) - 1
        return any(differs(S.full(f, g, 0, slots, wrong), S.full(f, g, 0, slots)) for f in frames)

    def retained(name, world, wrong):
        used.add(wrong)
        H = S.Histories(wrong)
        return [st.label for st in S.sequence(name, world) if differs(H.assemble("x", st.shards, st.geo, BG[st.bg], st.retained), S.expected(st))]

    def gather(name, world, wrong):
        used.add(wrong)
        g = S.geo_of(name, world)
        src, stride, off = S.compact_gather(g, seed=3)
        return differs(S.compact(src[off:], stride, g.table, g, wrong=wrong), S.compact(src[off:], stride, g.table, g))

    assert frame("71x45", 2, "half", "mode8", "no-quad-guard")                  # test_full_assembly[71x45]
    assert frame("71x45", 2, "half", "mode8", "no-row-guard") and frame("200x136", 3, "half", "opaque", "no-row-guard")
    assert frame("71x45", 1, "whole-tile", "mode8", "stride-is-width") and frame("100x64", 3, "half", "mode8", "stride-is-width")
    assert frame("100x64", 1, "full", "mode8", "no-npix-guard")                 # test_full_assembly[100x64]: the last tile row
    assert frame("128x128", 2, "cap-off", "mode8", "no-header-check") and frame("71x45", 3, "cpt-off", "opaque", "no-header-check")
    assert frame("128x128", 2, "stale-slots", "mode8", "slots-beyond-n") and frame("396x396", 8, "stale-slots", "opaque", "slots-beyond-n")
    assert one_short("71x45", 3, "n-not-clamped") and one_short("396x396", 3, "n-not-clamped")          # test_batch_and_prefixes
    assert frame("71x45", 1, "half", "opaque", "tail-is-bg") and frame("200x136", 8, "empty-shard", "opaque", "tail-is-bg")
    assert not frame("71x45", 1, "half", "mode8", "tail-is-bg")                 # (only the opaque convention can tell)
    for name, world in S.SEQUENCES:                                             # test_retained_sequences, test_retained_batches
        assert retained(name, world, "stale-is-seq") and retained(name, world, "no-stamp"), (name, world)
        assert "background changes" in retained(name, world, "background-survives"), (name, world)
    assert retained("128x128", 2, "grid-survives")[0] == "another grid"         # nothing before the grid changes, that step at once
    assert retained("71x45", 3, "clear-not-clipped") and retained("396x396", 3, "clear-not-clipped")    # partial cells beside lit ones
    assert not retained("128x128", 2, "clear-not-clipped")                     # (exact cells cannot tell)
    assert gather("128x128", 3, "padded-is-tile0") and gather("71x45", 8, "padded-is-tile0")            # test_compact
    assert gather("71x45", 2, "stride-is-width") and gather("100x64", 2, "no-npix-guard")
    assert used == set(S.WRONG) and len(S.WRONG) >= 12
    # the compact model leaves what no tile covers alone: the tail, and nothing else even where rows are sheared
    g = S.geo_of("71x45", 2)
    src, stride, off = S.compact_gather(g, seed=3)
    img = S.compact(src[off:], stride, g.table, g)
    assert (img[g.covered:] == S.PREFILL).all() and not (img[:g.covered] == S.PREFILL).any() and not S.has_sentinel(img)


@pytest.mark.parametrize("name,world", [(n, w) for n in ("128x128", "71x45", "200x136", "512x512", "100x64") for w in S.WORLDS])
def test_compact_gathers(name, world):
    g = S.geo_of(name, world)
    one, s1, o1 = S.compact_gather(g, seed=3)
    three, s3, o3 = S.compact_gather(g, seed=3, frames=3, frame=1)
    assert (s1, o1, s3, o3) == (g.shard_pixels, 0, 3 * g.shard_pixels, g.shard_pixels)
    a, b = S.compact(one, s1, g.table, g), S.compact(three[o3:], s3, g.table, g)
    np.testing.assert_array_equal(a, b)                                        # the same frame in the middle of three
    assert not S.has_sentinel(a) and (a[g.covered:] == S.PREFILL).all() and not (a[:g.covered] == S.PREFILL).any()
    assert ((g.table < 0).any()) == (S.SENT_FREE in one)
