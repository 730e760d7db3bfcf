"""GPU tests of frame assembly (csrc/vrt_assembly_kernel.hip behind csrc/vrt_hip_assembly.cpp) on crafted inputs: assemble_kernel,
scatter_sparse[_batch]_kernel and clear_stale_cells[_batch]_kernel against the numpy model of tests/assembly_scenes.py, whose scenes
tests/test_assembly_scenes.py checks on the CPU.

Nothing is rendered (but for the producer cross-check at the end): a context is given an image size, a tile grid and a shard, and is
handed shards made on the host -- cells in shuffled slots, sentinels in every free key and pixel slot and in the part of a stored cell
that lies outside its tile, headers that do not match, keys beyond the grid, prefixes of every kind the batch call accepts -- and frame
buffers prefilled with a value that is neither background nor sentinel.  Every comparison is exact, on all w * h words.

The inputs stay inside the two caller contracts of include/vrt_hip.h: shards are 16-byte aligned (torch allocations, strides that are
multiples of 4 words), and a prefix is one cell short of the fullest shard at most and is the header alone only when every shard is empty.
"""
import contextlib
import os

import numpy as np
import pytest

import assembly_scenes as S
from assembly_scenes import BG
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
VIEW = np.eye(4, dtype=np.float32)                        # any valid view: nothing is rendered


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def pack_of(pkg, bg):
    return pkg.PACK_ROUND | (pkg.ALPHA_COMPUTED if bg == "mode8" else pkg.ALPHA_OPAQUE)


def configure(r, geo):
    """The context assembles frames of `geo`; its own idea of the shard sizes must be the model's before anything is launched."""
    r.set_camera_view(geo.w, geo.h, VIEW)
    r.set_shard(0, geo.world)
    r.tile_gaussians_device(geo.tw, geo.th, VIEW, stream())
    assert r.sparse_shard_words() == geo.words and r.shard_pixels() == geo.shard_pixels, (r.sparse_shard_words(), r.shard_pixels(), geo)


@contextlib.contextmanager
def context(pkg, geo=None):
    from sgrt_amd import scene
    r = pkg.Renderer(0)
    try:
        r.set_gaussians(scene.grid_scene(1))
        if geo is not None:
            configure(r, geo)
        yield r
    finally:
        r.close()


def up(words):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def frame_buffers(n, npix):
    import torch
    return torch.full((n, npix), S.PREFILL, dtype=torch.int32, device="cuda")


def down(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def check(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=str(what))
    assert not S.has_sentinel(got), what


def batch_buffers(geo, frames, stride):
    """One device buffer per shard: [frame][stride words], and a whole shard of sentinels behind the last frame."""
    out = []
    for s in range(len(frames[0])):
        buf = np.full(len(frames) * stride + geo.words, S.SENT_FREE, np.uint32)
        for f, fr in enumerate(frames):
            buf[f * stride:(f + 1) * stride] = fr[s][:stride]
        out.append(up(buf))
    return out


@pytest.mark.parametrize("name", list(S.GEOMETRIES))
def test_full_assembly(pkg, name):
    """scatter_sparse_device at every geometry, world and background, with every kind of crafted frame."""
    with context(pkg) as r:
        for world in S.WORLDS + ((64,) if name == "32x32" else ()):
            geo = S.geo_of(name, world)
            configure(r, geo)
            img = frame_buffers(1, geo.npix)[0]
            for kind in S.KINDS if world <= 8 else ("half",):
                shards = S.frame_shards(geo, kind, seed=7)
                dev = [up(sh) for sh in shards]
                for bg in BG:
                    img.fill_(S.PREFILL)
                    r.scatter_sparse_device([d.data_ptr() for d in dev], pack_of(pkg, bg), img.data_ptr(), stream())
                    check(down(img), S.full(shards, geo, BG[bg]), (name, world, kind, bg))


@pytest.mark.parametrize("name,world,nframes", S.BATCH_CASES)
def test_batch_and_prefixes(pkg, name, world, nframes):
    """scatter_sparse_batch_device with the frame strides a gather may deliver: whole shards, the prefix of the fullest shard, one cell
    less (the last slot of the fullest shard is dropped: the caller gathers again), and the header alone with empty shards."""
    geo = S.geo_of(name, world)
    with context(pkg, geo) as r:
        images = frame_buffers(nframes, geo.npix)
        for label, stride, slots, frames in S.batch_strides(geo, S.batch_frames(geo, nframes, seed=11)):
            dev = batch_buffers(geo, frames, stride)
            for bg in BG:
                images.fill_(S.PREFILL)
                r.scatter_sparse_batch_device([d.data_ptr() for d in dev], stride, nframes, pack_of(pkg, bg), [im.data_ptr() for im in images], stream())
                got = down(images)
                for f in range(nframes):
                    check(got[f], S.full(frames[f], geo, BG[bg], slots), (name, world, label, bg, f))


def test_rejected_calls_touch_nothing(pkg):
    """0 and 65 frames, 65 shards, a stride that is no multiple of 4 words, two frames into one buffer, tiles of 0 pixels: each raises
    and leaves the frame buffers as they were; the context goes on working."""
    geo = S.geo_of("71x45", 2)
    with context(pkg, geo) as r:
        frames = S.batch_frames(geo, 2, seed=11)
        dev = batch_buffers(geo, frames, geo.words)
        ptrs, st, pack = [d.data_ptr() for d in dev], stream(), pack_of(pkg, "mode8")
        images = frame_buffers(65, geo.npix)
        im = [x.data_ptr() for x in images]
        for retained in (False, True):
            for args in ((ptrs, geo.words, 0, pack, im), (ptrs, geo.words, 65, pack, im), ([ptrs[0]] * 65, geo.words, 2, pack, im),
                         (ptrs, geo.words + 2, 2, pack, im), (ptrs, geo.words, 2, pack, [im[0], im[0]]), (ptrs, geo.words, 3, pack, [im[0], im[1], im[0]])):
                with pytest.raises(pkg.VrtHipError):
                    r.scatter_sparse_batch_device(*args, st, retained=retained)
            with pytest.raises(pkg.VrtHipError):
                r.scatter_sparse_device([ptrs[0]] * 65, pack, im[0], st, retained=retained)
        with pytest.raises(pkg.VrtHipError, match="one buffer"):
            r.scatter_sparse_batch_device(ptrs, geo.words, 2, pack, [im[1], im[1]], st, retained=True)
        assert (down(images) == S.PREFILL).all()
        for retained in (True, True, False):                      # and no rejected retained call left a history behind
            r.scatter_sparse_batch_device(ptrs, geo.words, 2, pack, im[:2], st, retained=retained)
            got = down(images)
            for f in range(2):
                check(got[f], S.full(frames[f], geo, 0), ("after the rejections", retained, f))
        assert (got[2:] == S.PREFILL).all()
    zero = S.geometry(4, 4, 0.25, 0.25, 1)
    with context(pkg, zero) as r:
        shard, images = up(np.array([0, 0, 0, 0], np.uint32)), frame_buffers(2, 16)
        for retained in (False, True):
            with pytest.raises(pkg.VrtHipError, match="0 pixels"):
                r.scatter_sparse_device([shard.data_ptr()], pack, images[0].data_ptr(), st, retained=retained)
            with pytest.raises(pkg.VrtHipError, match="0 pixels"):
                r.scatter_sparse_batch_device([shard.data_ptr()], 4, 2, pack, [x.data_ptr() for x in images], st, retained=retained)
        assert (down(images) == S.PREFILL).all()


@pytest.mark.parametrize("name,world", S.SEQUENCES)
def test_retained_sequences(pkg, name, world):
    """Crafted frames one after the other into one retained buffer: every step leaves what the full assembly would."""
    steps = S.sequence(name, world)
    with context(pkg) as r:
        geo, img = None, frame_buffers(1, steps[0].geo.npix)[0]
        for st in steps:
            if st.geo is not geo:
                geo = st.geo
                configure(r, geo)
            dev = [up(sh) for sh in st.shards]
            r.scatter_sparse_device([d.data_ptr() for d in dev], pack_of(pkg, st.bg), img.data_ptr(), stream(), retained=st.retained)
            check(down(img), S.expected(st), (name, world, st.label))


@pytest.mark.parametrize("name,world", S.SEQUENCES)
def test_retained_batches(pkg, name, world):
    """The same steps through the batch call, two frames a call into two buffers that swap places from call to call."""
    calls = S.alternating(name, world)
    with context(pkg) as r:
        geo, images = None, frame_buffers(2, calls[0][0][1].geo.npix)
        for (b0, s0), (b1, s1) in calls:
            if geo is None or s0.geo.sig != geo.sig:
                configure(r, s0.geo)
            geo = s0.geo
            dev = batch_buffers(geo, [s0.shards, s1.shards], geo.words)
            r.scatter_sparse_batch_device([d.data_ptr() for d in dev], geo.words, 2, pack_of(pkg, s0.bg), [images[b0].data_ptr(), images[b1].data_ptr()],
                                          stream(), retained=s0.retained)
            got = down(images)
            check(got[b0], S.expected(s0), (name, world, s0.label, "first frame"))
            check(got[b1], S.expected(s1), (name, world, s1.label, "second frame"))


@pytest.mark.parametrize("name", ["32x32", "64x32"])
def test_more_frame_buffers_than_histories(pkg, name):
    """64 retained buffers twice, a 65th, the first again, a retained batch of 64 new ones, batches of 32 old and 32 new: a context keeps
    64 histories, drops the oldest that is not part of the call, and every frame is the full assembly's all the same."""
    geo = S.geo_of(name, 1)
    with context(pkg, geo) as r:
        images = frame_buffers(129, geo.npix)
        want = np.full((129, geo.npix), S.PREFILL, np.uint32)
        pack, last = pack_of(pkg, "mode8"), 0
        for batch, bufs, rnd in S.history_ops():
            if batch or rnd != last:
                check(down(images), want, (name, "before round", rnd))
                last = rnd
            idx = [S.buffer_number(b) for b in bufs]
            frames = [S.history_frame(geo, i, rnd) for i in idx]
            if batch:
                dev = batch_buffers(geo, frames, geo.words)
                r.scatter_sparse_batch_device([d.data_ptr() for d in dev], geo.words, len(idx), pack, [images[i].data_ptr() for i in idx], stream(), retained=True)
            else:
                dev = up(frames[0][0])
                r.scatter_sparse_device([dev.data_ptr()], pack, images[idx[0]].data_ptr(), stream(), retained=True)
                down(dev)                                         # (the shard is freed when the loop goes on: wait for its assembly)
            for i, fr in zip(idx, frames):
                want[i] = S.full(fr, geo, 0)
        check(down(images), want, (name, "at the end"))


@pytest.mark.parametrize("name", ["128x128", "71x45", "200x136", "512x512", "100x64"])
def test_compact(pkg, name):
    """assemble_shards_device on gathers of seeded values with garbage in padded slots: one frame per rank, and the middle frame of
    three per rank; pixels that no tile covers keep what the buffer held."""
    with context(pkg) as r:
        for world in S.WORLDS:
            geo = S.geo_of(name, world)
            configure(r, geo)
            img = frame_buffers(1, geo.npix)[0]
            for nframes, frame in ((1, 0), (3, 1)):
                src, stride, off = S.compact_gather(geo, seed=3, frames=nframes, frame=frame)
                dev = up(src)
                img.fill_(S.PREFILL)
                r.assemble_shards_device(dev.data_ptr() + 4 * off, img.data_ptr(), stream(), rank_stride_px=None if nframes == 1 else stride)
                got = down(img)
                check(got, S.compact(src[off:], stride, geo.table, geo), (name, world, nframes))
                assert (got[geo.covered:] == S.PREFILL).all() and not (got[:geo.covered] == S.PREFILL).any()
        with pytest.raises(pkg.VrtHipError, match="rank stride"):
            r.assemble_shards_device(dev.data_ptr(), img.data_ptr(), stream(), rank_stride_px=geo.shard_pixels - 1)
        assert (down(img) == got).all()


@pytest.mark.parametrize("w,h,tiles_n", [(200, 136, 5), (100, 100, 16)])
@pytest.mark.parametrize("world", [2, 3])
def test_rendered_shards_through_the_model(pkg, renderer, w, h, tiles_n, world):
    """The one place a renderer is used: the sparse shards the ranks produce at truncated tile sizes (40 x 27-pixel tiles; 6-pixel tiles
    in rows of 96 of 100 pixels), brought back to the host and put through the model, give the single-context frame; every shard's
    header is the job's, and every cell is stored once, by the rank that owns its tile."""
    import torch
    from sgrt_amd import scene, sharding
    g = scene.read_obj(os.path.join(GOLDEN, "test-objects", "cube.obj"))
    cam, _ = scene.cli_camera(w, h, initial_rot=123.0)
    tw = 2.0 / tiles_n
    geo = S.geometry(w, h, tw, tw, world)
    assert geo.span < geo.npix and (geo.tiles_w, geo.tiles_h) == (tiles_n, tiles_n)              # a truncated tile size: no raster mirror applies
    st = stream()
    for bg in BG:
        pack = pack_of(pkg, bg)
        renderer.set_gaussians(g)
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        renderer.set_table_step(0.0)
        renderer.set_shard(0, 1)
        renderer.set_camera_view(w, h, cam.view)
        renderer.tile_gaussians(tw, tw, cam.view)
        want = renderer.render(cam.position, pack, want_radiance=False)[0].reshape(-1)
        assert (want != BG[bg]).sum() > 32 * 32
        ranks, host = [], []
        try:
            for rk in range(world):
                r = pkg.Renderer(0)
                ranks.append(r)
                r.set_gaussians(g)
                r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
                r.set_table_step(0.0)
                r.set_camera_view(w, h, cam.view)
                r.set_shard(rk, world)
                r.tile_gaussians_device(tw, tw, cam.view, st)
                assert r.sparse_shard_words() == geo.words
                buf = torch.full((geo.words,), -1, dtype=torch.int32, device="cuda")
                r.frame_sparse_call(tw, tw, cam.view, cam.position, pack)(buf.data_ptr(), st)
                host.append(down(buf))
        finally:
            for r in ranks:
                r.close()
        np.testing.assert_array_equal(S.full(host, geo, BG[bg]), want, err_msg=f"{bg}")
        keys = []
        for rk, sh in enumerate(host):
            assert tuple(sh[1:4]) == (geo.max_cells, geo.cpt, 0) and sh[0] <= geo.max_cells, (rk, sh[:4])
            mine = [int(k) for k in sh[S.HDR:S.HDR + int(sh[0])]]
            assert all(k < geo.frame_cells and sharding.shard_owner(k // geo.cpt, geo.tiles_w, world) == rk for k in mine), rk
            keys += mine
        assert len(keys) == len(set(keys)) > 0
