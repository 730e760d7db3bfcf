"""The kernels at their capacity limits, one element either side (scenes: tests/boundary_scenes.py; that the scenes can see a
lost or doubled element is checked on the CPU, tests/test_boundary_scenes.py).

Which kernel shades a block, and by which of its code paths, is decided by fixed capacities: PRUNE_PL 16, PL 24, light_cells 24,
dense_threshold = PCAP 96, the chunk size 64, TCAP 1024, DCAP 1024, TableCfg::TC 2048, cstride min(n, 4096), the chunk test by
default beyond 8192 Gaussians, MAX_FUSED_CELLS 64.  Every test renders lists of cap - 1, cap and cap + 1 against the oracle at the
project's own tolerances and reads from vrt_hip_stats that the path changed where the code says.

What the statistics count (vrt_hip_diag.cpp): `tile_entries` sums the length of the list a block STARTS from (its cell's, or its
tile's when the cell's slot overflowed) and `list_entries` the block's survivors, over every shaded block -- the block kernel adds
them for the blocks it shades itself (a block it hands over adds nothing there), the dense and the table kernel for theirs.
`lane_entries` / `lane_max_entries` (per-ray list lengths summed over rays / the longest per block summed over blocks) are the
block kernel's alone.  A block of the block kernel can never hold more than PCAP candidates: its cell holds at most
dense_threshold = PCAP = 96, so `pos < PCAP` / `cnt <= PCAP` there cannot be crossed from inside and no scene tries to.

PRUNE_PL here is the limit alone: WHICH entries the budgeted prune drops (the budget's edge, ties, every instantiation, the budget's
factors) and which a lane keeps in the first place are held decision by decision in tests/test_gpu_block.py (scenes and model:
tests/block_scenes.py).
"""
import numpy as np
import pytest

import boundary_scenes as B
from boundary_scenes import TOL

pytestmark = pytest.mark.gpu

PRUNE_BOUND = 2.46e-5   # what the ray-level prune may change (tests/test_gpu_parity.py, test_per_tile_cull_slack_keeps_the_error_bound)


def channels(img):
    img = np.asarray(img).reshape(-1)
    return ((img[:, None] >> np.array([0, 8, 16, 24], np.uint32)) & 255).astype(np.int32)


def load(r, sc):
    r.set_gaussians(sc.g)
    r.set_plane(sc.w, sc.h, *sc.plane)
    r.tile_gaussians(sc.tw, sc.th, sc.view)


def shoot(pkg, r, sc, eps, table_step, prune):
    """One frame with statistics: (packed pixels, radiance, stats) on the scene's checked pixels."""
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, eps)
    r.set_table_step(table_step)
    r.set_cull_prune(prune)
    r.enable_stats(True)
    img, rad = r.render(sc.origin)
    st = r.stats()
    return img.reshape(-1)[sc.pixels], rad.reshape(-1, 4)[sc.pixels].astype(np.float64), st


def restore(pkg, r):
    r.enable_stats(False)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    r.set_table_step(pkg.TABLE_STEP_DEFAULT)
    r.set_cull_prune(6.0)


def show(what, st, err=None):
    keys = ("shaded_blocks", "dense_blocks", "overflow_blocks", "table_blocks", "table_declined", "tile_entries", "list_entries",
            "lane_entries", "lane_max_entries")
    print(what, " ".join(f"{k}={st[k]}" for k in keys), "" if err is None else f"err={err:.3g}", flush=True)


@pytest.mark.parametrize("name,cap,n,w,h,chunked,compact", B.CLOUD_CASES, ids=[f"{c[0]}-{c[2]}" for c in B.CLOUD_CASES])
def test_all_visible_cloud_at_the_limit(pkg, oracle, renderer, name, cap, n, w, h, chunked, compact):
    """PL 24, DCAP = TCAP 1024, TableCfg::TC 2048: a 16x16 image (four blocks, one cell, one tile) whose every ray sees all n
    Gaussians with the culls off.  Lists up to PL are shaded by the block kernel (per ray and per block exactly n entries), one more
    and all four blocks are handed over (dense_blocks); more than DCAP survivors are streamed from scratch (overflow_blocks, exact
    kernels); the table kernel declines more than TC survivors.  Beyond TCAP the fused list kernel gives the cells no list of their
    own (count 0xFFFFFFFF) and the blocks read the tile's: no statistic tells, `tile_entries` is n per block either way -- there
    the markers at 0, 1023, 1024 and n - 1 against the oracle are the test.  Then the same scene at the default settings."""
    sc = B.cloud(oracle, cap, n, w, h, chunked, compact, npix=2 if n > 2000 else 3)
    oimg, orad = B.render_oracle(oracle, sc, threads=8)
    tol = B.tolerance(n, orad.max())
    blocks = (w // 8) * (h // 8)
    load(renderer, sc)
    try:
        for step in (0.0, pkg.TABLE_STEP_DEFAULT):
            img, rad, st = shoot(pkg, renderer, sc, 0.0, step, 0.0)
            err = np.abs(rad - orad).max()
            show(f"{name} n={n} culls off, table step {step:g}:", st, err)
            assert err <= tol, (step, err)
            assert np.abs(channels(img) - channels(oimg[sc.pixels])).max() <= 1
            assert st["shaded_blocks"] == blocks
            assert st["tile_entries"] == n * blocks and st["list_entries"] == n * blocks
            if n <= B.PL:
                assert st["dense_blocks"] == 0
                assert st["lane_entries"] == n * 64 * blocks and st["lane_max_entries"] == n * blocks
            else:
                assert st["dense_blocks"] == blocks and st["lane_entries"] == 0
            if step == 0.0:
                assert st["overflow_blocks"] == (blocks if n > B.DCAP else 0)
                assert st["table_blocks"] == 0
            else:
                assert st["table_blocks"] + st["table_declined"] == st["dense_blocks"]
                assert st["table_declined"] == (blocks if n > B.TABLE_TC else 0)
                assert st["overflow_blocks"] == (blocks if n > B.TABLE_TC else 0)     # a declined block is shaded by the exact body
        # the library's defaults: cull_eps 1e-9, table mode, prune factor 6 -- and the prune against the same context without it
        img, rad, st = shoot(pkg, renderer, sc, 1e-9, pkg.TABLE_STEP_DEFAULT, 6.0)
        _, rad0, _ = shoot(pkg, renderer, sc, 1e-9, pkg.TABLE_STEP_DEFAULT, 0.0)
        err = np.abs(rad - orad).max()
        show(f"{name} n={n} defaults:", st, err)
        assert err <= TOL, err
        assert np.abs(channels(img) - channels(oimg[sc.pixels])).max() <= 1
        assert np.abs(rad - rad0).max() <= PRUNE_BOUND
    finally:
        restore(pkg, renderer)


@pytest.mark.parametrize("name,cap,n,w,h,chunked,compact", B.CSTRIDE_CASES, ids=[f"cstride-{c[2]}" for c in B.CSTRIDE_CASES])
def test_cell_slot_at_cstride(pkg, oracle, renderer, name, cap, n, w, h, chunked, compact):
    """cstride = min(n, 4096) entries per cell slot.  The fused list kernel cannot get there: a tile list beyond TCAP = 1024 has
    already sent every cell to the tile's list.  build_cell_lists_kernel can -- tiles of more than 64 cells -- so: one tile of
    256 x 288 pixels (72 cells), 4095 / 4096 / 4097 narrow Gaussians around the view axis, every cull off.  Only the two cells that
    meet at the image centre hold them (all of them: `tile_entries` is n per shaded block); at 4096 the slot is full to its last
    entry, at 4097 the count saturates (0xFFFFFFFF) and the blocks read the tile's list.  No statistic tells the two apart: the markers at 0, 4095,
    4096 and n - 1 against the oracle do."""
    sc = B.cloud(oracle, cap, n, w, h, chunked, compact, npix=2)
    oimg, orad = B.render_oracle(oracle, sc, threads=8)
    tol = B.tolerance(n, orad.max())
    load(renderer, sc)
    try:
        for step in (0.0, pkg.TABLE_STEP_DEFAULT):
            img, rad, st = shoot(pkg, renderer, sc, 0.0, step, 0.0)
            err = np.abs(rad - orad).max()
            show(f"cstride n={n} culls off, table step {step:g}:", st, err)
            assert err <= tol, (step, err)
            assert np.abs(channels(img) - channels(oimg[sc.pixels])).max() <= 1
            # the two cells that meet at the image centre (the axis lies on their border), 16 blocks each, and nothing else
            assert st["shaded_blocks"] == st["dense_blocks"] == 32 and st["overflow_blocks"] > 0
            assert st["tile_entries"] == n * 32
    finally:
        restore(pkg, renderer)


@pytest.mark.parametrize("n", [B.PCAP - 1, B.PCAP, B.PCAP + 1])
def test_cell_list_at_the_dense_threshold(pkg, oracle, renderer, n):
    """dense_threshold = PCAP = 96 is a limit of the CELL's list.  (A block whose rays all see 25 or more is handed over whatever
    its cell holds, so the all-visible clouds never reach it inside the block kernel.)  One 32x32 cell with 95, 96 and 97 narrow
    Gaussians on a lattice, default culling, no ray keeps more than a handful: up to 96 the block kernel shades all 16 blocks from a
    list of n, at 97 the cell is filed in the dense queue."""
    sc = B.lattice(oracle, B.PCAP, n)
    oimg, orad = B.render_oracle(oracle, sc, threads=16)
    load(renderer, sc)
    try:
        for step in (0.0, pkg.TABLE_STEP_DEFAULT):
            rads = {}
            for prune in (0.0, 6.0):
                img, rad, st = shoot(pkg, renderer, sc, 1e-9, step, prune)
                rads[prune] = rad
                err = np.abs(rad - orad).max()
                show(f"lattice n={n} table step {step:g} prune {prune:g}:", st, err)
                assert err <= TOL, (step, prune, err)
                assert np.abs(channels(img) - channels(oimg)).max() <= 1
                assert st["shaded_blocks"] == 16 and st["tile_entries"] == 16 * n
                assert st["dense_blocks"] == (16 if n > B.PCAP else 0)
                assert st["lane_max_entries"] <= 16 * B.PL
            assert np.abs(rads[6.0] - rads[0.0]).max() <= PRUNE_BOUND
    finally:
        restore(pkg, renderer)


@pytest.mark.parametrize("n", [B.LIGHT_CELLS - 1, B.LIGHT_CELLS, B.LIGHT_CELLS + 1])
def test_cell_list_at_the_light_threshold(pkg, oracle, renderer, monkeypatch, n):
    """light_cells = 24: a cell with a list up to that long is filed from the BACK of the active queue.  No statistic shows the
    filing order; a cell filed wrongly (or twice, or not at all) shows in the image: against the oracle, and bit for bit against a
    context whose whole queue is drained by one wave (VRT_HIP_RENDER_GRID=1)."""
    sc = B.lattice(oracle, B.LIGHT_CELLS, n)
    oimg, orad = B.render_oracle(oracle, sc, threads=16)
    load(renderer, sc)
    try:
        img, rad, st = shoot(pkg, renderer, sc, 1e-9, pkg.TABLE_STEP_DEFAULT, 6.0)
        err = np.abs(rad - orad).max()
        show(f"light lattice n={n}:", st, err)
        assert err <= TOL, err
        assert np.abs(channels(img) - channels(oimg)).max() <= 1
        assert st["shaded_blocks"] == 16 and st["dense_blocks"] == 0 and st["tile_entries"] == 16 * n
        monkeypatch.setenv("VRT_HIP_RENDER_GRID", "1")
        r1 = pkg.Renderer(0)
        try:
            load(r1, sc)
            for _ in range(2):                        # both counter sets
                img1, rad1 = r1.render(sc.origin)
                np.testing.assert_array_equal(img1.reshape(-1), img)
                np.testing.assert_array_equal(rad1.reshape(-1, 4).astype(np.float64), rad)
        finally:
            r1.close()
    finally:
        restore(pkg, renderer)


def test_one_lane_over_the_per_ray_limit(pkg, oracle, renderer):
    """`fast = __ballot(nl > PL) == 0` is a per-wave decision from per-lane counts: 24 wide Gaussians every ray keeps plus a
    narrow one that only the ray of pixel (4, 4) keeps.  That lane's list is 25 long, so block 0 goes to the dense path; its three
    neighbours stay with the block kernel at exactly 24 per ray."""
    sc = B.one_lane_over(oracle)
    oimg, orad = B.render_oracle(oracle, sc, threads=16)
    load(renderer, sc)
    try:
        for step in (0.0, pkg.TABLE_STEP_DEFAULT):
            img, rad, st = shoot(pkg, renderer, sc, 1e-9, step, 6.0)
            err = np.abs(rad - orad).max()
            show(f"one lane over, table step {step:g}:", st, err)
            assert err <= TOL, (step, err)
            assert np.abs(channels(img) - channels(oimg)).max() <= 1
            assert st["shaded_blocks"] == 4 and st["dense_blocks"] == 1
            assert st["lane_max_entries"] == 3 * B.PL and st["lane_entries"] == 3 * 64 * B.PL
        # the narrow one does light its pixel: dropping it with the block would show
        assert np.abs(rad[sc.lane_pixel] - rad[sc.lane_pixel + 1]).max() > 100 * TOL
    finally:
        restore(pkg, renderer)


@pytest.mark.parametrize("n", [B.PRUNE_PL - 1, B.PRUNE_PL, B.PRUNE_PL + 1])
def test_prune_stops_at_its_list_length(pkg, oracle, renderer, n):
    """PRUNE_PL = 16 (`nmax <= PRUNE_PL`): n mutually visible Gaussians of which the last three are faint enough for the budgeted
    prune.  Lists of 15 and 16 lose entries against the run with the prune off, lists of 17 are left alone; every image stays
    within the prune's bound of the unpruned one and within the tolerance of the oracle."""
    sc = B.prunable(oracle, n)
    oimg, orad = B.render_oracle(oracle, sc, threads=16)
    load(renderer, sc)
    try:
        img0, rad0, st0 = shoot(pkg, renderer, sc, 1e-9, pkg.TABLE_STEP_DEFAULT, 0.0)
        img6, rad6, st6 = shoot(pkg, renderer, sc, 1e-9, pkg.TABLE_STEP_DEFAULT, 6.0)
        show(f"prune n={n} off:", st0, np.abs(rad0 - orad).max())
        show(f"prune n={n} on: ", st6, np.abs(rad6 - orad).max())
        assert st0["dense_blocks"] == 0 and st0["lane_entries"] == n * 256 and st0["lane_max_entries"] == n * 4
        if n <= B.PRUNE_PL:
            assert st6["lane_entries"] < st0["lane_entries"]
            assert st6["lane_entries"] >= (n - sc.faint) * 256          # nothing but the faint ones fits the budget
        else:
            assert st6["lane_entries"] == st0["lane_entries"] and st6["lane_max_entries"] == st0["lane_max_entries"]
        for img, rad in ((img0, rad0), (img6, rad6)):
            assert np.abs(rad - orad).max() <= TOL
            assert np.abs(channels(img) - channels(oimg)).max() <= 1
        assert np.abs(rad6 - rad0).max() <= PRUNE_BOUND
    finally:
        restore(pkg, renderer)


def _frame_of_a_fresh_context(pkg, sc, eps):
    r = pkg.Renderer(0)
    try:
        load(r, sc)
        r.set_options(pkg.EXP_VCL, pkg.ERF_AS, eps)
        r.enable_stats(True)
        img, rad = r.render(sc.origin)
        st = r.stats()
        return img, rad, st
    finally:
        r.close()


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129])
def test_chunk_test_with_full_and_ragged_last_chunks(pkg, oracle, monkeypatch, n):
    """The tile level's chunk test (runs of 64 consecutive Gaussians, VRT_HIP_CHUNKS=2) with a last chunk of 63, 64 and 1
    members: image, radiance and list statistics bit for bit those of the per-Gaussian pass (VRT_HIP_CHUNKS=0), with the culls off
    and at the default; markers on both sides of the chunk border and at both ends of the last chunk, against the oracle."""
    name, cap, _, w, h, chunked, compact = next(c for c in B.CHUNK_CASES if c[2] == n)
    sc = B.cloud(oracle, cap, n, w, h, chunked, compact)
    _, orad = B.render_oracle(oracle, sc, threads=8)
    for eps in (0.0, 1e-9):
        monkeypatch.setenv("VRT_HIP_CHUNKS", "0")
        img0, rad0, st0 = _frame_of_a_fresh_context(pkg, sc, eps)
        monkeypatch.setenv("VRT_HIP_CHUNKS", "2")
        img2, rad2, st2 = _frame_of_a_fresh_context(pkg, sc, eps)
        err = np.abs(rad2.reshape(-1, 4)[sc.pixels].astype(np.float64) - orad).max()
        show(f"chunks n={n} eps={eps:g}:", st2, err)
        np.testing.assert_array_equal(img2, img0)
        np.testing.assert_array_equal(rad2, rad0)
        assert st2["tile_entries"] == st0["tile_entries"] and st2["list_entries"] == st0["list_entries"]
        assert err <= TOL * max(1.0, float(orad.max()))
        if eps == 0.0:
            assert st2["tile_entries"] == 4 * n and st2["list_entries"] == 4 * n


@pytest.mark.parametrize("n", [B.CHUNKS_DEFAULT_N, B.CHUNKS_DEFAULT_N + 1])
def test_chunk_test_default_switch(pkg, oracle, monkeypatch, n):
    """Beyond 8192 Gaussians the chunk test is on by default (VRT_HIP_CHUNKS=1: `n > 8192`).  Out of the oracle's reach: GPU
    against GPU, the frame with the chunk test forbidden (VRT_HIP_CHUNKS=0) bit for bit, on both sides of the switch."""
    sc = B.cloud(oracle, B.CHUNKS_DEFAULT_N, n, 16, 16, chunked=True)
    monkeypatch.setenv("VRT_HIP_CHUNKS", "0")
    img0, rad0, st0 = _frame_of_a_fresh_context(pkg, sc, 1e-9)
    monkeypatch.setenv("VRT_HIP_CHUNKS", "1")
    img1, rad1, st1 = _frame_of_a_fresh_context(pkg, sc, 1e-9)
    show(f"chunks by default n={n}:", st1)
    np.testing.assert_array_equal(img1, img0)
    np.testing.assert_array_equal(rad1, rad0)
    assert st1["tile_entries"] == st0["tile_entries"] > 0 and st1["list_entries"] == st0["list_entries"] > 0
    assert rad1.max() > 0.05


@pytest.mark.parametrize("w,h,fused", [(256, 256, True), (256, 288, False)])
def test_tiles_of_64_and_of_more_cells(pkg, oracle, renderer, w, h, fused):
    """MAX_FUSED_CELLS = 64: one tile of 256 x 256 pixels (8 x 8 cells) goes through the fused list kernel, one of 256 x 288
    (72 cells) through the tile kernel and the one-wave-per-cell kernel; the same 300 Gaussians at the image centre, against the
    oracle on the lit pixels.  A frame batch accepts the first and refuses the second (VRT_HIP_ERR_INVALID = -1)."""
    import torch
    sc = B.cloud(oracle, 256, 300, w, h, compact=True, npix=6)
    oimg, orad = B.render_oracle(oracle, sc, threads=8)
    assert orad.min() > 0.01                              # lit pixels
    load(renderer, sc)
    try:
        for step in (0.0, pkg.TABLE_STEP_DEFAULT):
            img, rad, st = shoot(pkg, renderer, sc, 1e-9, step, 6.0)
            err = np.abs(rad - orad).max()
            show(f"{w}x{h} table step {step:g}:", st, err)
            assert err <= TOL * max(1.0, float(orad.max())), (step, err)
            assert np.abs(channels(img) - channels(oimg[sc.pixels])).max() <= 1
    finally:
        restore(pkg, renderer)
    r = pkg.Renderer(0)
    try:
        r.set_gaussians(sc.g)
        r.set_camera_view(w, h, sc.view)
        out = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        call = r.frame_batch_call([], 2.0, 2.0, [sc.view], [sc.origin], pkg.PACK_ROUND | pkg.ALPHA_COMPUTED)
        if fused:
            call([out.data_ptr()], st)
            torch.cuda.synchronize()
            r.tile_gaussians(2.0, 2.0, sc.view)
            ref, _ = r.render(sc.origin, want_radiance=False)
            np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ref.reshape(-1))
            assert (ref.reshape(-1)[sc.pixels] >> 24).min() > 0
        else:
            with pytest.raises(pkg.VrtHipError, match=r"\(-1\).*64 cells"):
                call([out.data_ptr()], st)
            # the batch was refused by its planning, after the context had advanced its generations: a single frame through the
            # same context right behind it is still right
            r.frame_call(2.0, 2.0, sc.view, sc.origin, pkg.PACK_ROUND | pkg.ALPHA_COMPUTED)(out.data_ptr(), st)
            torch.cuda.synchronize()
            r.tile_gaussians(2.0, 2.0, sc.view)
            ref, _ = r.render(sc.origin, want_radiance=False)
            np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ref.reshape(-1))
            assert (ref.reshape(-1)[sc.pixels] >> 24).min() > 0
    finally:
        r.close()


@pytest.mark.parametrize("w,h", [(96, 64), (100, 100)])
def test_tiles_that_are_not_square(pkg, oracle, renderer, w, h):
    """tw != th (4 x 3 tiles): every other test and fuzzer passes the same number twice.  Tile counts and indices against the
    oracle's tile_gaussians, the frame against the oracle on every pixel the reference writes (its truncated tile size,
    rt.h:348-349, as in test_ragged_geometry)."""
    tw, th = 2.0 / 4, 2.0 / 3
    g = oracle.grid_scene(6)
    cam, _ = oracle.cli_camera(w, h)
    plane, view, origin = oracle.camera_plane(cam), oracle.camera_view(cam), np.array(cam.position[:], np.float32)
    renderer.set_gaussians(g)
    renderer.set_plane(w, h, *plane)
    renderer.tile_gaussians(tw, th, view)
    tiles = oracle.tile_gaussians(tw, th, g, view)
    assert (tiles["w"], tiles["h"]) == (4, 3)
    counts = renderer.tile_counts()
    assert counts.shape == (3, 4)
    np.testing.assert_array_equal(counts.ravel(), np.diff(tiles["offsets"])[:12])
    for t in range(12):
        np.testing.assert_array_equal(renderer.tile_indices(t), tiles["indices"][tiles["offsets"][t]:tiles["offsets"][t + 1]])
    try:
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        img, rad = renderer.render(origin)
        tile_w, tile_h = int(np.float32(w) * tiles["tw"] / np.float32(2)), int(np.float32(h) * tiles["th"] / np.float32(2))
        n_written = tile_w * tiles["w"] * tile_h * tiles["h"]
        pix = np.arange(min(n_written, w * h), dtype=np.uint32)
        oimg, orad = oracle.render(w, h, plane, origin, g, tiles, pixels=pix, threads=16)
        assert orad.max() > 0.01
        assert np.abs(rad.reshape(-1, 4)[pix] - orad).max() <= TOL
        assert np.abs(channels(img.reshape(-1)[pix]) - channels(oimg[pix])).max() <= 1
        assert (img.reshape(-1)[len(pix):] == 0).all()
    finally:
        restore(pkg, renderer)
