"""GPU tests of the multi-GPU path on ONE GPU: several contexts / group members on device 0 stand for the ranks.

  - sparse shards (vrt_hip_frame_sparse_device) of 2, 3 and 8 "ranks", scattered by vrt_hip_scatter_sparse_device, give
    the single-context frame bit for bit -- sparse scenes, dense scenes (cells of the dense queue), table mode,
    tile sizes that are not a multiple of the 32-px cell, more ranks than tiles, both background conventions;
  - the device-side shard layout is the one sharding.py mirrors on the host (the gloo tests use that mirror);
  - vrt_hip_group (what `volumetric-ray-tracer --gpus N` drives) with members on one device; frames back to back;
  - the CLI with --gpus 2 (VRT_HIP_DEVICES=0,0): same PNG as one GPU, frame-parallel animation runs;
  - bench.py's N = 2 flow over gloo on one GPU.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "simd-gaussian-ray-tracing_amd", "bin")
OBJ = os.path.join(GOLDEN, "test-objects")


def single_frame(pkg, r, g, cam, w, h, tiles_n, pack, table=0.0):
    r.set_gaussians(g)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    r.set_table_step(table)
    r.set_shard(0, 1)
    r.set_camera_view(w, h, cam.view)
    r.tile_gaussians(2.0 / tiles_n, 2.0 / tiles_n, cam.view)
    img, _ = r.render(cam.position, pack, want_radiance=False)
    return img


@pytest.mark.parametrize("scene_name,w,h,tiles_n,world,rot,table", [
    ("g64", 1024, 1024, 16, 2, 0.0, 0.0),        # sparse scene: 95 % background
    ("g64", 1024, 1024, 16, 8, 47.0, 0.0),       # seen at an angle: dense cells appear
    ("monkey", 512, 512, 16, 3, 20.0, 0.0),      # dense kernel for most cells
    ("monkey", 512, 512, 16, 2, 20.0, 0.05),     # table kernel (the default step) + exact kernel behind it
    ("monkey", 512, 512, 16, 2, 20.0, 0.12),     # a coarser step: second attempts, declined blocks
    ("cube", 200, 136, 5, 3, 123.0, 0.0),        # 40 x 27-px tiles: partial cells; truncated tile size
    ("g4", 96, 96, 2, 8, 0.0, 0.0),              # more ranks than tiles
])
@pytest.mark.parametrize("pack_name", ["mode8", "opaque"])
def test_sparse_shards_assemble_to_the_single_gpu_frame(pkg, renderer, scene_name, w, h, tiles_n, world, rot, table, pack_name):
    import torch
    from sgrt_amd import scene, sharding
    g = {"g64": lambda: scene.grid_scene(64), "g4": lambda: scene.grid_scene(4),
         "monkey": lambda: scene.read_obj(os.path.join(OBJ, "monkey.obj")),
         "cube": lambda: scene.read_obj(os.path.join(OBJ, "cube.obj"))}[scene_name]()
    pack = pkg.PACK_ROUND | (pkg.ALPHA_COMPUTED if pack_name == "mode8" else pkg.ALPHA_OPAQUE)
    cam, _ = scene.cli_camera(w, h, initial_rot=rot)
    want = single_frame(pkg, renderer, g, cam, w, h, tiles_n, pack, table)
    st = torch.cuda.current_stream().cuda_stream
    ranks, shards = [], []
    try:
        for rk in range(world):
            r = pkg.Renderer(0)
            ranks.append(r)
            r.set_gaussians(g)
            r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
            r.set_table_step(table)
            r.set_camera_view(w, h, cam.view)
            r.set_shard(rk, world)
            r.tile_gaussians_device(2.0 / tiles_n, 2.0 / tiles_n, cam.view, st)
            words = r.sparse_shard_words()
            buf = torch.full((words,), -1, dtype=torch.int32, device="cuda")     # garbage: only what is written may be used
            r.frame_sparse_call(2.0 / tiles_n, 2.0 / tiles_n, cam.view, cam.position, pack)(buf.data_ptr(), st)
            shards.append(buf)
        out = torch.full((w * h,), 0x55, dtype=torch.int32, device="cuda")
        ranks[0].scatter_sparse_device([b.data_ptr() for b in shards], pack, out.data_ptr(), st)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32).reshape(h, w)
        np.testing.assert_array_equal(got, want)
        # the device layout is the one the host mirror reads (sharding.scatter_sparse), and the cells partition the lit area
        host = [b.cpu().numpy().view(np.uint32) for b in shards]
        tile_w, tile_h = int(np.float32(w) * np.float32(2.0 / tiles_n) / np.float32(2.0)), int(np.float32(h) * np.float32(2.0 / tiles_n) / np.float32(2.0))
        bg = 0 if pack_name == "mode8" else 0xFF000000
        if tile_w * tiles_n == w and tile_h * tiles_n == h:
            np.testing.assert_array_equal(sharding.scatter_sparse(host, tiles_n, tile_w, tile_h, h, w, background=bg), want)
        stored = sum(int(s[0]) for s in host)
        caps = {int(s[1]) for s in host if int(s[1])}
        assert len(caps) <= 1                                        # one capacity for the whole job
        keys = np.concatenate([s[4:4 + int(s[0])] for s in host])
        assert len(np.unique(keys)) == stored                        # no cell stored twice
        if scene_name == "g64" and rot == 0.0:
            assert stored * 1024 < 0.2 * w * h                       # the point of the format: most of the frame never travels
    finally:
        for r in ranks:
            r.close()


def test_retained_assembly_equals_full_assembly(pkg, renderer):
    """vrt_hip_scatter_sparse_retained_device: a frame buffer that keeps the previous assembly gets only the cells that went
    dark reset -- frame after frame of a moving camera it must hold exactly what the full assembly (background fill +
    cells) writes; a buffer, background or image-size change in between starts over by itself."""
    import torch
    from sgrt_amd import scene
    g = scene.grid_scene(16)
    world, tiles_n = 3, 8
    st = torch.cuda.current_stream().cuda_stream
    ranks = []
    try:
        for rk in range(world):
            r = pkg.Renderer(0)
            r.set_gaussians(g)
            r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
            r.set_shard(rk, world)
            ranks.append(r)
        bufs = {}
        steps = [(512, 0.0, "mode8", 0), (512, 9.0, "mode8", 0), (512, 31.0, "mode8", 0), (512, 31.0, "mode8", 0), (512, 77.0, "mode8", 0),
                 (512, 80.0, "opaque", 0), (512, 95.0, "opaque", 0), (512, 95.0, "opaque", 1), (512, 120.0, "opaque", 1),
                 (384, 120.0, "opaque", 0), (384, 160.0, "opaque", 0), (512, 10.0, "mode8", 0), (512, 200.0, "mode8", 0)]
        lit = set()
        for w, rot, pack_name, which in steps:
            pack = pkg.PACK_ROUND | (pkg.ALPHA_COMPUTED if pack_name == "mode8" else pkg.ALPHA_OPAQUE)
            cam, _ = scene.cli_camera(w, w, initial_rot=rot)
            shards = []
            for r in ranks:
                r.set_camera_view(w, w, cam.view)
                r.tile_gaussians_device(2.0 / tiles_n, 2.0 / tiles_n, cam.view, st)
                buf = torch.zeros(r.sparse_shard_words(), dtype=torch.int32, device="cuda")
                r.frame_sparse_call(2.0 / tiles_n, 2.0 / tiles_n, cam.view, cam.position, pack)(buf.data_ptr(), st)
                shards.append(buf)
            ptrs = [b.data_ptr() for b in shards]
            want = torch.full((w * w,), 0x77, dtype=torch.int32, device="cuda")
            ranks[0].scatter_sparse_device(ptrs, pack, want.data_ptr(), st)
            # the retained buffers live as long as the test: one per (size, which) -- a smaller image after a larger one
            # takes another buffer, as a caller's would
            key = (w, which)
            if key not in bufs:
                bufs[key] = torch.full((w * w,), 0x11, dtype=torch.int32, device="cuda")
            got = bufs[key]
            ranks[0].scatter_sparse_device(ptrs, pack, got.data_ptr(), st, retained=True)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=f"{(w, rot, pack_name, which)}")
            lit.add(int((want != (0 if pack_name == "mode8" else -16777216)).sum().item()))
        assert len(lit) > 3                                  # the lit area really changed between frames
    finally:
        for r in ranks:
            r.close()


def test_batch_assembly_equals_frame_by_frame(pkg, renderer):
    """vrt_hip_scatter_sparse_batch_device: F frames from [rank][frame][words] buffers into F frame buffers with one launch,
    retained per buffer -- three rounds of moving cameras, every frame equal to its plain assembly."""
    import torch
    from sgrt_amd import scene
    g = scene.grid_scene(16)
    world, tiles_n, F, w = 3, 8, 3, 384
    pack = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    st = torch.cuda.current_stream().cuda_stream
    ranks = []
    try:
        for rk in range(world):
            r = pkg.Renderer(0)
            r.set_gaussians(g)
            r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
            r.set_shard(rk, world)
            ranks.append(r)
        cam0, _ = scene.cli_camera(w, w)
        for r in ranks:
            r.set_camera_view(w, w, cam0.view)
            r.tile_gaussians_device(2.0 / tiles_n, 2.0 / tiles_n, cam0.view, st)
        words = ranks[0].sparse_shard_words()
        assert words % 4 == 0
        bufs = [torch.zeros(F * words, dtype=torch.int32, device="cuda") for _ in range(world)]
        images = [torch.full((w * w,), 0x11, dtype=torch.int32, device="cuda") for _ in range(F)]
        for rnd in range(3):
            want = []
            for f in range(F):
                cam, _ = scene.cli_camera(w, w, initial_rot=50.0 * rnd + 13.0 * f)
                for r, b in zip(ranks, bufs):
                    r.set_camera_view(w, w, cam.view)
                    r.frame_sparse_call(2.0 / tiles_n, 2.0 / tiles_n, cam.view, cam.position, pack)(b.data_ptr() + 4 * f * words, st)
                full = torch.full((w * w,), 0x77, dtype=torch.int32, device="cuda")
                ranks[0].scatter_sparse_device([b.data_ptr() + 4 * f * words for b in bufs], pack, full.data_ptr(), st)
                want.append(full)
            ranks[0].scatter_sparse_batch_device([b.data_ptr() for b in bufs], words, F, pack, [im.data_ptr() for im in images], st, retained=True)
            torch.cuda.synchronize()
            for f in range(F):
                np.testing.assert_array_equal(images[f].cpu().numpy(), want[f].cpu().numpy(), err_msg=f"round {rnd} frame {f}")
        with pytest.raises(pkg.VrtHipError, match="one buffer"):
            ranks[0].scatter_sparse_batch_device([b.data_ptr() for b in bufs], words, 2, pack, [images[0].data_ptr()] * 2, st)
    finally:
        for r in ranks:
            r.close()


def test_group_frames_on_one_device(pkg, renderer):
    """vrt_hip_group with 1, 2 and 3 members on device 0: group_frame == the single-context frame; a second frame with
    another camera enqueued right behind the first (shard buffers are reused: the group orders that itself)."""
    from sgrt_amd import scene
    w = h = 768
    g = scene.grid_scene(64)
    pack = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    cams = [scene.cli_camera(w, h, initial_rot=a)[0] for a in (0.0, 33.0, 0.0)]
    want = [single_frame(pkg, renderer, g, c, w, h, 16, pack) for c in cams]
    for n in (1, 2, 3):
        grp = pkg.Group([0] * n)
        try:
            for m in grp.members:
                m.set_gaussians(g)
                m.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
            for c, ref in zip(cams, want):
                for m in grp.members:
                    m.set_camera_view(w, h, c.view)
                grp.frame(2 / 16, 2 / 16, c.view, c.position, pack, want_image=False, wait=False)     # not waited for
                got = grp.frame(2 / 16, 2 / 16, c.view, c.position, pack)
                np.testing.assert_array_equal(got, ref)
        finally:
            grp.close()


@pytest.mark.parametrize("scene_name,w,n_members", [("g64", 768, 3), ("monkey", 256, 2)])
def test_group_frame_batches_on_one_device(pkg, renderer, scene_name, w, n_members):
    """vrt_hip_group_frame_batch: the orbit's next cameras handed over at once -- one launch of each kernel per member and
    one assembly launch per batch.  Every frame equals the single-context frame, bit for bit: batches back to back (the
    retained frame buffers), a shorter batch, a scene change in between (the mirror contexts follow the member's own
    context), and a single group_frame afterwards."""
    from sgrt_amd import scene
    h = w
    g = scene.grid_scene(64) if scene_name == "g64" else scene.read_obj(os.path.join(OBJ, scene_name + ".obj"))
    g2 = scene.grid_scene(16)
    pack = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    cams = [scene.cli_camera(w, h, initial_rot=11.0 * k)[0] for k in range(7)]
    want = [single_frame(pkg, renderer, g, c, w, h, 16, pack, table=pkg.TABLE_STEP_DEFAULT) for c in cams]
    want2 = [single_frame(pkg, renderer, g2, c, w, h, 16, pack, table=pkg.TABLE_STEP_DEFAULT) for c in cams[:3]]
    grp = pkg.Group([0] * n_members)
    try:
        for m in grp.members:
            m.set_gaussians(g)
            m.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
            m.set_camera_view(w, h, cams[0].view)
        for lo, hi in ((0, 4), (4, 7), (1, 3)):
            got = grp.frame_batch(2 / 16, 2 / 16, [c.view for c in cams[lo:hi]], [c.position for c in cams[lo:hi]], pack)
            for k in range(lo, hi):
                np.testing.assert_array_equal(got[k - lo], want[k], err_msg=f"frames {lo}..{hi}: frame {k}")
        for m in grp.members:
            m.set_gaussians(g2)
        got = grp.frame_batch(2 / 16, 2 / 16, [c.view for c in cams[:3]], [c.position for c in cams[:3]], pack)
        for k in range(3):
            np.testing.assert_array_equal(got[k], want2[k], err_msg=f"after the scene change: frame {k}")
        for m in grp.members:
            m.set_camera_view(w, h, cams[2].view)
        np.testing.assert_array_equal(grp.frame(2 / 16, 2 / 16, cams[2].view, cams[2].position, pack), want2[2])
    finally:
        grp.close()


def test_group_frames_survive_a_resize_between_unwaited_frames(pkg, renderer):
    """Round-2 advisor: the group frees a member's shard buffer when the image grows; the previous frame's assembly on
    member 0's stream may still be reading it when that frame was not waited for."""
    from sgrt_amd import scene
    g = scene.grid_scene(64)
    pack = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    grp = pkg.Group([0, 0])
    try:
        for m in grp.members:
            m.set_gaussians(g)
            m.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        for w, tiles_n in ((512, 16), (1024, 16), (1024, 8), (2048, 16), (256, 4)):
            cam = scene.cli_camera(w, w, initial_rot=20.0)[0]
            want = single_frame(pkg, renderer, g, cam, w, w, tiles_n, pack, table=pkg.TABLE_STEP_DEFAULT)
            for m in grp.members:
                m.set_camera_view(w, w, cam.view)
            grp.frame(2 / tiles_n, 2 / tiles_n, cam.view, cam.position, pack, want_image=False, wait=False)
            grp.frame(2 / tiles_n, 2 / tiles_n, cam.view, cam.position, pack, want_image=False, wait=False)
            np.testing.assert_array_equal(grp.frame(2 / tiles_n, 2 / tiles_n, cam.view, cam.position, pack), want, err_msg=f"{w} px, {tiles_n} tiles")
    finally:
        grp.close()


def test_cli_gpus_flag(tmp_path):
    """--gpus 2 with both members on GPU 0: the tile-sharded single frame writes the PNG one GPU writes; the animation
    without output deals whole frames to the members and prints the average."""
    from PIL import Image
    exe = os.path.join(BIN, "volumetric-ray-tracer")
    env = dict(os.environ, VRT_HIP_DEVICES="0,0")
    for args in (["-g", "16", "-w", "512", "-i", "20"], ["-f", os.path.join(OBJ, "sphere.obj"), "-w", "256", "--tiles", "8"]):
        a = subprocess.run([exe, *args, "-q", "-o", "one.png"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        b = subprocess.run([exe, *args, "-q", "--gpus", "2", "-o", "two.png"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
        assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
        assert b.stdout.startswith("TIME: ")
        np.testing.assert_array_equal(np.array(Image.open(tmp_path / "one.png")), np.array(Image.open(tmp_path / "two.png")))
    p = subprocess.run([exe, "-g", "64", "-w", "1024", "-q", "--gpus", "2", "--frames", "24"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0 and p.stdout.startswith("AVG. TIME: ") and "(24 frames)" in p.stdout, p.stdout + p.stderr
    q = subprocess.run([exe, "-g", "8", "-w", "128", "-q", "--gpus", "2", "--frames", "3", "-o", "f.png"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300, env=env)
    assert q.returncode == 0 and all((tmp_path / f"f_{k}.png").exists() for k in (1, 2, 3)), q.stderr
    # an orbit that writes its frames goes through the group in batches (vrt_hip_group_frame_batch): the frames one GPU writes,
    # with 4 members on one device and batches of 5 (the last one shorter)
    env4 = dict(os.environ, VRT_HIP_DEVICES="0,0,0,0", VRT_CLI_GROUP_BATCH="5")
    a = subprocess.run([exe, "-g", "64", "-w", "512", "-q", "--frames", "12", "-r", "90", "-o", "s.png"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    b = subprocess.run([exe, "-g", "64", "-w", "512", "-q", "--frames", "12", "-r", "90", "--gpus", "4", "-o", "m.png"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300, env=env4)
    assert a.returncode == 0 and b.returncode == 0 and "AVG. TIME: " in b.stdout and "(12 frames)" in b.stdout, a.stderr + b.stderr
    for k in range(1, 13):
        np.testing.assert_array_equal(np.array(Image.open(tmp_path / f"s_{k}.png")), np.array(Image.open(tmp_path / f"m_{k}.png")), err_msg=f"frame {k}")


def _free_port():
    """a port nobody listens on (a fixed one can still be in TIME_WAIT from an earlier run on the same box)"""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def test_bench_two_ranks_rehearsal_on_one_gpu(tmp_path):
    """bench.py's N = 2 flow (sparse shards -> gather -> scatter on rank 0) with the gloo backend, both ranks on GPU 0:
    the assembled frame must equal the single-GPU frame (bench.py checks it and reports it in its JSON line)."""
    env = dict(os.environ, VRT_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5",   # what the driver times
           "--width", "1024", "--no-cpu-baseline", "--full"]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2 and res["config"]["frame_equals_single_gpu_frame"] is True
    # a short run takes smaller gather batches: rendering, gather and assembly of different batches overlap as in a long one
    assert res["config"]["gather_batches_in_timed_region"] >= 3 and res["config"]["frames_per_gather"] == 5
    assert res["config"]["shard_transport"]["bytes_per_frame"] < 0.25 * 1024 * 1024 * 4
    # what torch.distributed saw, and where each rank's time went (round-3 verdict: make a miss of the first real run attributable)
    col = res["collective"]
    assert col["backend"] == "gloo" and col["world_size"] == 2 and [pr["rank"] for pr in col["per_rank"]] == [0, 1]
    for pr in col["per_rank"]:
        assert pr["render_ms_per_frame"] > 0 and pr["gather_ms_per_frame_upper_bound"] > 0 and pr["host_ms_per_frame_in_loop"] > 0
        assert pr["batches_gathered_twice"] == res["config"]["shard_transport"]["batches_gathered_twice"] or pr["rank"] != 0
    assert col["per_rank"][0]["assemble_ms_per_frame"] > 0 and col["per_rank"][1]["assemble_ms_per_frame"] == 0
    # the control beside it: whole frames on every rank, no exchange (N x one GPU by construction; here both ranks share one GPU)
    ctl = col["frame_parallel_control"]
    assert ctl["scaling"] == "weak" and ctl["value"] > 0 and len(ctl["ms_per_rank"]) == 2 and all(v > 0 for v in ctl["ms_per_rank"])
