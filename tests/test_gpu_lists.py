"""The list kernels (csrc/vrt_kernels.hip) on their own: every cell's list against a float64 model.  The fused kernel
(build_tile_lists_body: chunk_test, filter_cells, file_cells, clear_empty_cells), the unfused pair (build_tile_lists_kernel +
build_cell_lists_kernel) and the cone table hand every shading kernel its input; image parity does not see a cull that is a little too
tight (1e-5 of a pixel) and nothing sees one that is too loose (longer lists, the same pixels).  Scenes, the model and its margins:
tests/list_scenes.py; that the scenes can see ten wrong variants of the model: tests/test_list_scenes.py.

Per frame (a view of a cloud, a path -- device binning, caller-made lists, no tiles --, cull_eps, Exp kind, cull_ref_n):
  raster      table step 0 and the default, statistics on: shaded_blocks and tile_entries EQUAL the model's (every inside block of every
              non-empty cell, and the length of the list it starts from); dense_blocks equals the model's where no ray of a cell that
              is not dense can keep more than PL, else it is at least the model's.  Every pixel of a cell the model calls empty is
              exactly the background, with computed and with opaque alpha; a seeded sample of lit pixels is within TOL max(1, peak) of
              the oracle.
  sparse      (device binning: vrt_hip_frame_sparse_device bins itself) the shard of rank 0 of 1 into a buffer of garbage: header word 0
              is the number of non-empty cells, the keys are exactly the model's set, none twice, dense cells included; light filing is
              off there, and the stored cells scatter to the raster frame bit for bit.
No tolerance is invented: counts are equalities, the background is exact, pixels use the project's TOL.  Every frame is rendered
with the block kernel's budgeted prune off (set_cull_prune(0)): the prune is held by tests/test_gpu_block.py, it changes none of the
counts here, and its documented bound (3 kappa 1365 cull_eps: 2.5e-3 at cull_eps = 1e-7) is not the parity tolerance's business.
The unfused pair of tiles (2 x 1 tiles of 288 x 272 pixels) makes the one image wider than 288 pixels: 576 x 272.
"""
import numpy as np
import pytest

import list_scenes as S

pytestmark = pytest.mark.gpu

CHUNK_CASES = [("grid", S.GRID_FRAMES[-1]), ("grid-rows", S.frame(S.GRID_VIEW, chunks=True))]


def exp_kind(pkg, fr):
    return {"vcl": pkg.EXP_VCL, "libm": pkg.EXP_LIBM}[fr.exp]


def load(pkg, oracle, r, cloud, fr):
    sc = S.view_of(oracle, cloud, fr.view)
    r.set_gaussians(sc.g)
    r.set_plane(sc.w, sc.h, *sc.plane)
    r.set_shard(0, 1)
    if fr.mode == "device":
        r.tile_gaussians(sc.tw, sc.th, sc.view)
    elif fr.mode == "none":
        r.clear_tiles()
    else:
        lists = S.frame_lists(oracle, cloud, fr)
        off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
        r.set_tiles(dict(sc.ref, offsets=off, indices=np.concatenate(lists).astype(np.uint32)))
    return sc


def shoot(pkg, r, sc, fr, step, pack, want_radiance=True):
    r.set_options(exp_kind(pkg, fr), pkg.ERF_AS, fr.eps)
    r.set_table_step(step)
    r.set_cull_prune(0.0)       # the block kernel's budgeted prune has a suite of its own: what differs from the oracle here is the lists'
    r.enable_stats(True)
    img, rad = r.render(sc.origin, pack, want_radiance=want_radiance)
    return img.reshape(-1).copy(), (rad.reshape(-1, 4).astype(np.float64) if want_radiance else None), r.stats()


def restore(pkg, r):
    r.enable_stats(False)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    r.set_table_step(pkg.TABLE_STEP_DEFAULT)
    r.set_cull_prune(6.0)


def hold_counts(what, st, p):
    print(what, " ".join(f"{k}={st[k]}" for k in ("shaded_blocks", "tile_entries", "dense_blocks", "list_entries")),
          f"| model: shaded_blocks={p.shaded_blocks} tile_entries={p.tile_entries} dense_blocks{'=' if p.dense_exact else '>='}{p.dense_blocks}", flush=True)
    assert st["shaded_blocks"] == p.shaded_blocks, (what, st["shaded_blocks"], p.shaded_blocks)
    assert st["tile_entries"] == p.tile_entries, (what, st["tile_entries"], p.tile_entries)
    if p.dense_exact:
        assert st["dense_blocks"] == p.dense_blocks, (what, st["dense_blocks"], p.dense_blocks)
    else:
        assert st["dense_blocks"] >= p.dense_blocks, (what, st["dense_blocks"], p.dense_blocks)


def empty_pixels(p):
    keys = sorted({c.key for c in p.cells} - p.cells_lit)
    return np.concatenate([S.cell_pixels(p.L, k) for k in keys]) if keys else np.zeros(0, np.int64)


def raster_frames(pkg, oracle, r, cloud, fr, sc, p):
    """Table step 0 and default, computed and opaque alpha.  Returns the default frame with computed alpha."""
    what = f"{cloud.name}-{fr.name}"
    dark = empty_pixels(p)
    pix, orad, peak = S.lit_sample(oracle, cloud, fr, p)
    computed, opaque = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED, pkg.PACK_ROUND | pkg.ALPHA_OPAQUE
    for step in (0.0, pkg.TABLE_STEP_DEFAULT):
        img, rad, st = shoot(pkg, r, sc, fr, step, computed)
        hold_counts(f"{what} step {step:g}:", st, p)
        assert (img[dark] == 0).all() and (rad[dark] == 0.0).all(), what
        err = np.abs(rad[pix] - orad).max()
        print(f"{what} step {step:g}: {len(pix)} lit pixels, largest error against the oracle {err:.3g} (tolerance {S.TOL * peak:.3g}); {len(dark)} empty pixels", flush=True)
        assert err <= S.TOL * peak, (what, step, float(err))
        img_o, _, st_o = shoot(pkg, r, sc, fr, step, opaque, want_radiance=False)
        hold_counts(f"{what} step {step:g} opaque:", st_o, p)
        assert (img_o[dark] == 0xFF000000).all(), what
        assert ((img_o & 0xFFFFFF) == (img & 0xFFFFFF)).all(), what
    return img


def sparse_frame(pkg, r, sc, fr, p, raster):
    """The sparse shard of the same frame (light filing off): header, keys, and the scattered cells against the raster frame."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    pack = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    r.tile_gaussians_device(sc.tw, sc.th, sc.view, st)
    buf = torch.full((r.sparse_shard_words(),), -1, dtype=torch.int32, device="cuda")      # garbage: only what is written may be used
    r.frame_sparse_call(sc.tw, sc.th, sc.view, sc.origin, pack)(buf.data_ptr(), st)
    out = torch.full((sc.w * sc.h,), 0x55, dtype=torch.int32, device="cuda")
    r.scatter_sparse_device([buf.data_ptr()], pack, out.data_ptr(), st)
    torch.cuda.synchronize()
    shard = buf.cpu().numpy().view(np.uint32)
    stored = int(shard[0])
    assert stored == len(p.cells_lit), (stored, len(p.cells_lit))
    assert int(shard[2]) == p.L.cpt and stored <= int(shard[1])
    keys = shard[4:4 + stored]
    assert len(np.unique(keys)) == stored
    assert set(keys.tolist()) == p.cells_lit, (sorted(set(keys.tolist()) - p.cells_lit), sorted(p.cells_lit - set(keys.tolist())))
    assert {c.key for c in p.cells if c.cls == S.DENSE} <= set(keys.tolist())
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), raster)


def run_frame(pkg, oracle, r, name, fr):
    cloud = S.cloud(oracle, name)
    sc = load(pkg, oracle, r, cloud, fr)
    p = S.plan_frame(oracle, cloud, fr)
    assert p.unsure == 0
    raster = raster_frames(pkg, oracle, r, cloud, fr, sc, p)
    if fr.mode == "device":
        q = S.plan_frame(oracle, cloud, fr, light=False)
        assert S.observables(q) == S.observables(p)
        sparse_frame(pkg, r, sc, fr, q, raster)


@pytest.mark.parametrize("name,fr", S.CASES, ids=S.CASE_IDS)
def test_lists(pkg, oracle, renderer, monkeypatch, name, fr):
    """Every frame of tests/list_scenes.py: the grid, partial cells and blocks, TCAP in one tile of several (fused) and the same cloud
    unfused, a negative cell slack, caller-made lists (one with a Gaussian taken out by hand), no tiles, no refine, the thresholds."""
    if fr.ref_n == 0:
        monkeypatch.setenv("VRT_HIP_CULL_REF_N", "0")
        r = pkg.Renderer(0)
    else:
        r = renderer
    try:
        run_frame(pkg, oracle, r, name, fr)
    finally:
        if r is renderer:
            restore(pkg, r)
        else:
            r.close()


@pytest.mark.parametrize("name,fr", CHUNK_CASES, ids=["scene-order", "raster-rows"])
def test_chunks_change_nothing(pkg, oracle, monkeypatch, name, fr):
    """VRT_HIP_CHUNKS=2: the tile level tests the bounding spheres of 64 consecutive Gaussians first.  The model knows nothing of
    chunks; a radius that is a hair too small shows as a missing entry.  Spheres that span the scene, and tight ones."""
    monkeypatch.setenv("VRT_HIP_CHUNKS", "2")
    r = pkg.Renderer(0)
    try:
        run_frame(pkg, oracle, r, name, fr)
    finally:
        r.close()


def test_queue_order_does_not_matter(pkg, oracle, renderer, monkeypatch):
    """Queue positions across tiles come from atomics.  VRT_HIP_RENDER_GRID=1: one wave drains the queues, in their order; the frame is
    bit for bit the default's."""
    cloud, fr = S.cloud(oracle, "grid"), S.GRID_FRAMES[0]
    p = S.plan_frame(oracle, cloud, fr)
    pack = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    monkeypatch.setenv("VRT_HIP_RENDER_GRID", "1")
    one = pkg.Renderer(0)
    try:
        sc = load(pkg, oracle, renderer, cloud, fr)
        img, rad, st = shoot(pkg, renderer, sc, fr, pkg.TABLE_STEP_DEFAULT, pack)
        load(pkg, oracle, one, cloud, fr)
        img1, rad1, st1 = shoot(pkg, one, sc, fr, pkg.TABLE_STEP_DEFAULT, pack)
        hold_counts("default grid:", st, p)
        hold_counts("one wave:", st1, p)
        np.testing.assert_array_equal(img1, img)
        np.testing.assert_array_equal(rad1, rad)
    finally:
        one.close()
        restore(pkg, renderer)


def test_cone_table(pkg, oracle):
    """One context: camera A; A again after another cull_eps and back (lists rebuilt, cones read from the table); camera B (new tag, the
    rows are rebuilt); A again.  Every frame has the model's numbers for its camera and is bit for bit a fresh context's."""
    cloud = S.cloud(oracle, "grid-cameras")
    fa, fb = cloud.frames
    pack = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    fresh = {}
    for fr in (fa, fb):
        r = pkg.Renderer(0)
        try:
            fresh[fr.name] = shoot(pkg, r, load(pkg, oracle, r, cloud, fr), fr, pkg.TABLE_STEP_DEFAULT, pack)
        finally:
            r.close()
    r = pkg.Renderer(0)
    try:
        sc = load(pkg, oracle, r, cloud, fa)
        frames = [("A", fa, shoot(pkg, r, sc, fa, pkg.TABLE_STEP_DEFAULT, pack))]
        shoot(pkg, r, sc, S.frame(fa.view, eps=S.EPS_TEST), pkg.TABLE_STEP_DEFAULT, pack)
        frames.append(("A after another cull_eps", fa, shoot(pkg, r, sc, fa, pkg.TABLE_STEP_DEFAULT, pack)))
        frames.append(("B", fb, shoot(pkg, r, load(pkg, oracle, r, cloud, fb), fb, pkg.TABLE_STEP_DEFAULT, pack)))
        frames.append(("A again", fa, shoot(pkg, r, load(pkg, oracle, r, cloud, fa), fa, pkg.TABLE_STEP_DEFAULT, pack)))
        for what, fr, (img, rad, st) in frames:
            hold_counts(f"cone table, {what}:", st, S.plan_frame(oracle, cloud, fr))
            np.testing.assert_array_equal(img, fresh[fr.name][0], err_msg=what)
            np.testing.assert_array_equal(rad, fresh[fr.name][1], err_msg=what)
    finally:
        r.close()
