"""Host frames (vrt_hip_host_register / vrt_hip_frame_host / vrt_hip_host_unregister): frames delivered into a caller's
registered host buffer, only the cells that changed in that buffer since its last delivery.  Every frame must equal a fresh
render of its pose, whatever the buffer received before.  These are the workload's frames; which words each delivery writes and
leaves alone is checked cell by cell, on crafted cases against a model, in tests/test_gpu_host_frame_cells.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
SENTINEL = 0x12345678


def fresh(pkg, renderer, g, cam, w, tiles_n, pack):
    """A fresh vrt_hip_render of the pose: the reference every delivered frame is held to."""
    renderer.set_gaussians(g)
    renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    renderer.set_camera_view(w, w, cam.view)
    renderer.tile_gaussians(2.0 / tiles_n, 2.0 / tiles_n, cam.view)
    return renderer.render(cam.position, pack, want_radiance=False)[0]


def delivered(buf, w, h):
    return buf.reshape(-1)[:w * h].reshape(h, w).copy()


def deliver(r, buf, cam, w, tiles_n, pack):
    r.set_camera_view(w, w, cam.view)
    r.frame_host(2 / tiles_n, 2 / tiles_n, cam.view, cam.position, pack, buf)
    r.sync()
    return delivered(buf, w, w)


def test_host_frames_equal_fresh_frames_over_a_long_lived_buffer(pkg, renderer):
    """The step list of test_retained_frame_buffer_equals_fresh_frames through frame_host into ONE registered buffer: orbit,
    the same view twice, 768 -> 512, opaque <-> computed alpha, 16 <-> 8 tiles, a render in between, three scenes, and
    w = 500 (tiles that do not cover the image: the full copy carries the uncovered pixels).  Every step is compared."""
    from sgrt_amd import scene
    scenes = {"g64": scene.grid_scene(64), "g16": scene.grid_scene(16), "monkey": scene.read_obj(os.path.join(GOLDEN, "test-objects", "monkey.obj"))}
    mode8, opaque = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED, pkg.PACK_TRUNC | pkg.ALPHA_OPAQUE
    steps = [("g64", 768, 16, mode8, 0.0), ("g64", 768, 16, mode8, 10.0), ("g64", 768, 16, mode8, 10.0), ("g64", 768, 16, mode8, 55.0),
             ("g64", 768, 16, mode8, 0.0), ("g64", 512, 16, mode8, 0.0), ("g64", 512, 16, opaque, 0.0), ("g64", 512, 16, opaque, 30.0),
             ("g64", 512, 8, opaque, 30.0), ("g64", 512, 8, mode8, 31.0), ("render", 512, 8, mode8, 31.0), ("g64", 512, 8, mode8, 32.0),
             ("g16", 512, 8, mode8, 32.0), ("monkey", 512, 8, mode8, 32.0), ("monkey", 512, 8, mode8, 200.0), ("g16", 500, 16, mode8, 5.0),
             ("g16", 500, 16, mode8, 50.0), ("g64", 768, 16, mode8, 0.0)]
    r = pkg.Renderer(0)
    buf = pkg.host_frame(768, 768)
    buf[:] = 0x7F7F7F7F        # garbage: the first delivery must overwrite all of it
    r.register_host(buf)
    try:
        cur = None
        for k, (name, w, tiles_n, pack, rot) in enumerate(steps):
            cam = scene.cli_camera(w, w, initial_rot=rot)[0]
            if name == "render":   # another image into the context's own buffer, by another entry point
                r.set_camera_view(w, w, cam.view)
                r.tile_gaussians(2 / tiles_n, 2 / tiles_n, cam.view)
                r.render(cam.position, pack, want_radiance=False)
                continue
            if name != cur:
                r.set_gaussians(scenes[name]); cur = name
            got = deliver(r, buf, cam, w, tiles_n, pack)
            want = fresh(pkg, renderer, scenes[name], cam, w, tiles_n, pack)
            np.testing.assert_array_equal(got, want, err_msg=f"step {k}: {name} {w} px, {tiles_n} tiles, rot {rot}")
    finally:
        r.close()


def test_delta_delivery_writes_only_changed_cells(pkg, renderer, monkeypatch):
    """A delta delivery leaves a cell alone that is background now and was background at the buffer's last delivery: a
    sentinel there survives, one in a lit cell is overwritten.  After re-registration (history restarted) and on a context
    without stamps (VRT_HIP_RETAIN_FRAME=0) the delivery is a full copy: both sentinels are overwritten."""
    from sgrt_amd import scene
    g = scene.grid_scene(16)
    w, tiles_n, pack = 1024, 16, pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    cam = scene.cli_camera(w, w)[0]
    want = fresh(pkg, renderer, g, cam, w, tiles_n, pack)
    corner = (5, 5)                                       # cell 0 of tile 0: the grid covers the central fifth of the view
    assert want[corner] == 0
    lit = np.unravel_index(int(np.argmax(want >> 24)), want.shape)   # a pixel with coverage: its cell is lit
    assert want[lit] != 0

    def sentinels_after_redelivery(r, buf):
        buf[corner] = SENTINEL
        buf[lit] = SENTINEL
        got = deliver(r, buf, cam, w, tiles_n, pack)
        return got[corner], got[lit]

    r = pkg.Renderer(0)
    try:
        r.set_gaussians(g)
        buf = pkg.host_frame(w, w)
        r.register_host(buf)
        np.testing.assert_array_equal(deliver(r, buf, cam, w, tiles_n, pack), want)     # full (first delivery)
        np.testing.assert_array_equal(deliver(r, buf, cam, w, tiles_n, pack), want)     # delta
        bg_px, lit_px = sentinels_after_redelivery(r, buf)
        assert bg_px == SENTINEL, "a cell dark now and at the last delivery was written: no delta delivery"
        assert lit_px == want[lit]
        r.unregister_host(buf)
        r.register_host(buf)
        bg_px, lit_px = sentinels_after_redelivery(r, buf)
        assert bg_px == want[corner] and lit_px == want[lit], "the first delivery after registration must be a full one"
    finally:
        r.close()

    monkeypatch.setenv("VRT_HIP_RETAIN_FRAME", "0")
    r0 = pkg.Renderer(0)
    monkeypatch.delenv("VRT_HIP_RETAIN_FRAME")
    try:
        r0.set_gaussians(g)
        buf = pkg.host_frame(w, w)
        r0.register_host(buf)
        deliver(r0, buf, cam, w, tiles_n, pack)
        np.testing.assert_array_equal(deliver(r0, buf, cam, w, tiles_n, pack), want)
        bg_px, lit_px = sentinels_after_redelivery(r0, buf)
        assert bg_px == want[corner] and lit_px == want[lit], "without stamps every delivery must be a full one"
    finally:
        r0.close()


def test_frames_without_delivery_in_between(pkg, renderer):
    """Deliver; then three frames with moving poses and no delivery (one of them looks away from the scene: every cell
    dark) and a vrt_hip_render; then deliver again: the buffer's history is its own, the result equals a fresh render."""
    from sgrt_amd import scene
    g = scene.grid_scene(16)
    w, tiles_n, pack = 1024, 16, pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    r = pkg.Renderer(0)
    try:
        r.set_gaussians(g)
        buf = pkg.host_frame(w, w)
        r.register_host(buf)
        cam = scene.cli_camera(w, w)[0]
        deliver(r, buf, cam, w, tiles_n, pack)
        away = scene.Camera((0.0, 0.0, -4.0), w, w, 90.0, 0.0, 1.0)     # looks along -z, away from the grid at z = 1
        for c in (scene.cli_camera(w, w, initial_rot=20.0)[0], scene.cli_camera(w, w, initial_rot=-35.0)[0]):
            r.set_camera_view(w, w, c.view)
            r.frame(2 / tiles_n, 2 / tiles_n, c.view, c.position, pack, want_image=False, wait=False)
        r.set_camera_view(w, w, away.view)
        assert not r.frame(2 / tiles_n, 2 / tiles_n, away.view, away.position, pack).any()
        c = scene.cli_camera(w, w, initial_rot=-30.0)[0]
        r.set_camera_view(w, w, c.view)
        r.tile_gaussians(2 / tiles_n, 2 / tiles_n, c.view)
        r.render(c.position, pack, want_radiance=False)
        for rot in (40.0, 45.0):
            cam = scene.cli_camera(w, w, initial_rot=rot)[0]
            np.testing.assert_array_equal(deliver(r, buf, cam, w, tiles_n, pack), fresh(pkg, renderer, g, cam, w, tiles_n, pack),
                                          err_msg=f"rot {rot}")
    finally:
        r.close()


def test_ring_of_buffers_with_frames_in_flight(pkg, renderer):
    """4 contexts with 2 registered buffers each; 16 orbit frames of -g 16 -w 1024 in large steps (cells light up and go
    dark), enqueued round-robin; a context is synchronised only when its buffer comes round again.  Every frame == fresh."""
    from sgrt_amd import scene
    g = scene.grid_scene(16)
    w, tiles_n, pack, n = 1024, 16, pkg.PACK_ROUND | pkg.ALPHA_COMPUTED, 16
    poses = []
    cam, angle = scene.cli_camera(w, w)
    for _ in range(n):
        poses.append((cam.view.copy(), cam.position.copy()))
        angle = scene.orbit_step(cam, angle, 23.0)
    wants = []
    for view, pos in poses:
        renderer.set_gaussians(g)
        renderer.set_camera_view(w, w, view)
        renderer.tile_gaussians(2 / tiles_n, 2 / tiles_n, view)
        wants.append(renderer.render(pos, pack, want_radiance=False)[0])
    ctxs = [pkg.Renderer(0) for _ in range(4)]
    try:
        bufs = []
        for r in ctxs:
            r.set_gaussians(g)
            pair = [pkg.host_frame(w, w), pkg.host_frame(w, w)]
            for b in pair:
                r.register_host(b)
            bufs.append(pair)
        pending = {}
        for k, (view, pos) in enumerate(poses):
            ci, bi = k % 4, (k // 4) % 2
            if (ci, bi) in pending:            # the buffer comes round again: its frame must have landed
                ctxs[ci].sync()
                j = pending.pop((ci, bi))
                np.testing.assert_array_equal(delivered(bufs[ci][bi], w, w), wants[j], err_msg=f"frame {j}")
            ctxs[ci].set_camera_view(w, w, view)
            ctxs[ci].frame_host(2 / tiles_n, 2 / tiles_n, view, pos, pack, bufs[ci][bi])
            pending[(ci, bi)] = k
        for r in ctxs:
            r.sync()
        for (ci, bi), j in pending.items():
            np.testing.assert_array_equal(delivered(bufs[ci][bi], w, w), wants[j], err_msg=f"frame {j}")
    finally:
        for r in ctxs:
            r.close()


@pytest.mark.parametrize("table_step", [None, 0.0])
def test_dense_and_table_frames(pkg, table_step):
    """Teapot 512^2 (dense cells: table kernel by default, exact dense kernel with table step 0): delivered == frame()."""
    from sgrt_amd import scene
    g = scene.read_obj(os.path.join(GOLDEN, "test-objects", "teapot.obj"))
    w, tiles_n, pack = 512, 16, pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    r = pkg.Renderer(0)
    try:
        r.set_gaussians(g)
        if table_step is not None:
            r.set_table_step(table_step)
        buf = pkg.host_frame(w, w)
        r.register_host(buf)
        for rot in (0.0, 15.0):
            cam = scene.cli_camera(w, w, initial_rot=rot)[0]
            got = deliver(r, buf, cam, w, tiles_n, pack)
            want = r.frame(2 / tiles_n, 2 / tiles_n, cam.view, cam.position, pack)
            np.testing.assert_array_equal(got, want, err_msg=f"rot {rot}")
    finally:
        r.close()


@pytest.mark.parametrize("w", [250, 100])
def test_widths_without_aligned_rows(pkg, w):
    """16 tiles at w = 250 / 100: tile rows not 16-byte aligned, partial cells, columns no tile covers."""
    from sgrt_amd import scene
    g = scene.grid_scene(16)
    tiles_n, pack = 16, pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    r = pkg.Renderer(0)
    try:
        r.set_gaussians(g)
        buf = pkg.host_frame(w, w)
        r.register_host(buf)
        for rot in (0.0, 30.0, 31.0):
            cam = scene.cli_camera(w, w, initial_rot=rot)[0]
            got = deliver(r, buf, cam, w, tiles_n, pack)
            want = r.frame(2 / tiles_n, 2 / tiles_n, cam.view, cam.position, pack)
            np.testing.assert_array_equal(got, want, err_msg=f"rot {rot}")
    finally:
        r.close()


def test_refusals_and_lifetime(pkg, renderer):
    """Host-side refusals (nothing enqueued): an unregistered or too-small buffer, a buffer registered twice (with this or
    another context), a misaligned pointer.  unregister_host after an unsynced frame_host returns once the frame landed;
    close() with buffers still registered succeeds."""
    from sgrt_amd import scene
    g = scene.grid_scene(16)
    w, tiles_n, pack = 256, 16, pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    cam = scene.cli_camera(w, w)[0]
    want = fresh(pkg, renderer, g, cam, w, tiles_n, pack)
    r, r2 = pkg.Renderer(0), pkg.Renderer(0)
    try:
        r.set_gaussians(g)
        r.set_camera_view(w, w, cam.view)
        args = (2 / tiles_n, 2 / tiles_n, cam.view, cam.position, pack)
        with pytest.raises(pkg.VrtHipError, match="not registered"):
            r.frame_host(*args, pkg.host_frame(w, w))
        small = pkg.host_frame(64, 64)
        r.register_host(small)
        with pytest.raises(pkg.VrtHipError, match="fewer pixels"):
            r.frame_host(*args, small)
        buf = pkg.host_frame(w, w)
        r.register_host(buf)
        with pytest.raises(pkg.VrtHipError, match="already registered"):
            r.register_host(buf)
        with pytest.raises(pkg.VrtHipError, match="already registered"):
            r2.register_host(buf)
        with pytest.raises(pkg.VrtHipError, match="aligned"):
            r2.register_host(pkg.host_frame(w, w).reshape(-1)[1:])
        with pytest.raises(pkg.VrtHipError, match="not registered"):
            r2.frame_host(*args, buf)                  # registered, but with another context
        r.frame_host(*args, buf)
        r.unregister_host(buf)                         # waits for the delivery
        np.testing.assert_array_equal(delivered(buf, w, w), want)
        r.register_host(buf)
        r.frame_host(*args, buf)
    finally:
        r.close()                                      # buffers still registered (one with a frame in flight)
        r2.close()
    np.testing.assert_array_equal(delivered(buf, w, w), want)


def test_cli_written_frames_equal_python_frames(pkg, tmp_path):
    """volumetric-ray-tracer -g 16 -w 1024 --frames 6 -r 300 -o orbit.png delivers each frame into its registered host
    buffer: the PNGs decode to the frames of the Python path at the same poses (mode 8: u32 A|R|G|B little-endian)."""
    from PIL import Image
    from sgrt_amd import scene
    exe = os.path.join(ROOT, "simd-gaussian-ray-tracing_amd", "bin", "volumetric-ray-tracer")
    p = subprocess.run([exe, "-g", "16", "-w", "1024", "-q", "--frames", "6", "-r", "300", "-o", "orbit.png"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.startswith("AVG. TIME: "), p.stdout
    w, tiles_n, pack = 1024, 16, pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
    r = pkg.Renderer(0)
    try:
        r.set_gaussians(scene.grid_scene(16))
        cam, angle = scene.cli_camera(w, w)
        for k in range(1, 7):
            r.set_camera_view(w, w, cam.view)
            want = r.frame(2 / tiles_n, 2 / tiles_n, cam.view, cam.position, pack)
            png = np.array(Image.open(tmp_path / f"orbit_{k}.png"))
            np.testing.assert_array_equal(png, want.view(np.uint8).reshape(w, w, 4), err_msg=f"frame {k}")
            angle = scene.orbit_step(cam, angle, 300.0 / 6)
    finally:
        r.close()
