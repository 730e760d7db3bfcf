"""Frame delivery into host memory (vrt_hip_frame_host) against frames that stay on the device and against the pageable
copy of vrt_hip_frame(image_out).  Host clock around work that ends in a synchronisation, after warm-up, medians.

    python tools/host_delivery.py [--out profiles/host_delivery.json]       one JSON line (and the file)
    python tools/host_delivery.py --trace                                    the delivery workload alone, for
        rocprofv3 --kernel-trace --stats -- python tools/host_delivery.py --trace   (the delivery kernel's time)

Figures (ms per frame unless named otherwise):
  d2h_pinned_GBps         a 16.8 MB device -> pinned-host copy (torch, non_blocking): the host link as this box gives it
  headline_{static,moving}: -g 64 -w 2048 (16 tiles, mode 8), camera still / orbiting 1 degree per frame, serial:
      device   vrt_hip_frame(image_out = NULL, wait)      pageable   vrt_hip_frame(image_out = preallocated numpy array)
      delta    frame_host + sync                          full       frame_host + sync on a context without stamps
                                                                     (VRT_HIP_RETAIN_FRAME=0: every delivery a full copy)
  pipelined: 400 frames over 4 contexts, each with its own registered buffer (device-only for comparison)
  cfg3 (teapot 2048^2) and cfg5 (24 consecutive monkey 4096^2 orbit frames): device / delta / full
  cells_written: cells the delta deliveries wrote (from the frames: cells with a non-background pixel now, plus cells
      that had one at the previous delivery), per frame -- with the kernel time of a rocprofv3 run, its GB/s
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge._load_pkg()
from sgrt_amd import scene  # noqa: E402

PACK = pkg.PACK_ROUND | pkg.ALPHA_COMPUTED
TILES = 16
OBJ = os.path.join(ROOT, "tests", "golden", "test-objects")


def med(xs):
    return round(float(np.median(xs)), 4)


def make(g, retain=True):
    if not retain:
        os.environ["VRT_HIP_RETAIN_FRAME"] = "0"   # read once, by vrt_hip_create
    try:
        r = pkg.Renderer(0)
    finally:
        os.environ.pop("VRT_HIP_RETAIN_FRAME", None)
    r.set_gaussians(g)
    return r


def poses(w, n, rot0=0.0, step=0.0):
    cam, angle = scene.cli_camera(w, w, initial_rot=rot0)
    out = []
    for _ in range(n):
        out.append((cam.view.copy(), cam.position.copy()))
        if step:
            angle = scene.orbit_step(cam, angle, step)
    return out


def serial(r, w, ps, kind, buf=None, warm=3):
    """ms per frame, each frame set up, rendered (and delivered) and waited for; median over the poses after `warm`."""
    L, h = r._L, r._h
    ts = []
    for k, (view, pos) in enumerate(ps):
        t0 = time.perf_counter()
        r.set_camera_view(w, w, view)
        if kind == "device":
            r.frame(2 / TILES, 2 / TILES, view, pos, PACK, want_image=False, wait=True)
        elif kind == "pageable":   # the C call with a preallocated array: what the CLI did per written frame
            v = np.ascontiguousarray(view, np.float32)
            o = np.ascontiguousarray(pos, np.float32)
            rc = L.vrt_hip_frame(h, 2 / TILES, 2 / TILES, pkg._fp(v), pkg._fp(o), PACK, buf.ctypes.data, 1)
            assert rc == 0
        else:
            r.frame_host(2 / TILES, 2 / TILES, view, pos, PACK, buf)
            r.sync()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return med(ts)


def four_paths(g, w, ps, warm=3, paths=("device", "pageable", "delta", "full")):
    out = {}
    for kind in paths:
        r = make(g, retain=kind != "full")
        buf = pkg.host_frame(w, w) if kind != "device" else None
        if kind in ("delta", "full"):
            r.register_host(buf)
        out[kind] = serial(r, w, ps, kind, buf, warm)
        r.close()
    return out


def cells_written(g, w, ps):
    """Cells the delta path writes per frame, from the frames themselves (non-background cells now and at the last delivery)."""
    r = make(g)
    prev, counts = None, []
    for view, pos in ps:
        r.set_camera_view(w, w, view)
        img = r.frame(2 / TILES, 2 / TILES, view, pos, PACK)
        cw = int(w * np.float32(2 / TILES) / np.float32(2))   # tile width (w divisible by TILES here: cells tile the image)
        assert cw * TILES == w
        lit = (img.reshape(w // 32, 32, w // 32, 32) != 0).any(axis=(1, 3))
        counts.append(int(lit.sum() if prev is None else (lit | prev).sum()))
        prev = lit
    r.close()
    return counts


def d2h_pinned_GBps(nbytes, n=30):
    import torch
    d = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    hbuf = torch.empty(nbytes // 4, dtype=torch.int32, pin_memory=True)
    for _ in range(3):
        hbuf.copy_(d, non_blocking=True)
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        hbuf.copy_(d, non_blocking=True)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(nbytes / float(np.median(ts)) / 1e9, 2), round(float(np.median(ts)) * 1e3, 4)


def pipelined(g, w, n=400, nctx=4, host=True):
    ctxs = [make(g) for _ in range(nctx)]
    bufs = []
    for r in ctxs:
        b = pkg.host_frame(w, w)
        if host:
            r.register_host(b)
        bufs.append(b)
        r.set_camera_view(w, w, poses(w, 1)[0][0])
    view, pos = poses(w, 1)[0]

    def run(frames):
        for k in range(frames):
            r = ctxs[k % nctx]
            if host:
                r.frame_host(2 / TILES, 2 / TILES, view, pos, PACK, bufs[k % nctx])
            else:
                r.frame(2 / TILES, 2 / TILES, view, pos, PACK, want_image=False, wait=False)
        for r in ctxs:
            r.sync()
    run(4 * nctx)
    t0 = time.perf_counter()
    run(n)
    ms = (time.perf_counter() - t0) * 1e3 / n
    for r in ctxs:
        r.close()
    return round(ms, 4)


def trace_workload():
    """What rocprofv3 times: headline deliveries (static, then moving) and the cfg5 orbit, delta path."""
    g64 = scene.grid_scene(64)
    for ps in (poses(2048, 60), poses(2048, 60, step=1.0)):
        r = make(g64)
        b = pkg.host_frame(2048, 2048)
        r.register_host(b)
        serial(r, 2048, ps, "delta", b)
        r.close()
    mk = scene.read_obj(os.path.join(OBJ, "monkey.obj"))
    r = make(mk)
    b = pkg.host_frame(4096, 4096)
    r.register_host(b)
    serial(r, 4096, poses(4096, 24, rot0=176.0, step=1.0), "delta", b)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.trace:
        trace_workload()
        return
    res = {"what": "ms per frame (host clock, medians) of frames delivered into host memory; see tools/host_delivery.py"}
    res["d2h_pinned_GBps"], res["d2h_pinned_16.8MB_ms"] = d2h_pinned_GBps(2048 * 2048 * 4)
    res["d2h_pinned_67MB_GBps"], res["d2h_pinned_67MB_ms"] = d2h_pinned_GBps(4096 * 4096 * 4)
    g64 = scene.grid_scene(64)
    res["headline_static"] = four_paths(g64, 2048, poses(2048, 33))
    res["headline_moving"] = four_paths(g64, 2048, poses(2048, 33, step=1.0))
    res["headline_cells_written_static"] = med(cells_written(g64, 2048, poses(2048, 4)))
    res["headline_cells_written_moving"] = med(cells_written(g64, 2048, poses(2048, 24, step=1.0))[1:])
    res["pipelined_4ctx_host"] = pipelined(g64, 2048)
    res["pipelined_4ctx_device"] = pipelined(g64, 2048, host=False)
    tp = scene.read_obj(os.path.join(OBJ, "teapot.obj"))
    res["cfg3_teapot_2048"] = four_paths(tp, 2048, poses(2048, 23), paths=("device", "delta", "full"))
    res["cfg3_cells_written"] = med(cells_written(tp, 2048, poses(2048, 2)))
    mk = scene.read_obj(os.path.join(OBJ, "monkey.obj"))
    res["cfg5_monkey_4096_orbit24"] = four_paths(mk, 4096, poses(4096, 24, rot0=176.0, step=1.0), warm=2,
                                                 paths=("device", "delta", "full"))
    res["cfg5_cells_written"] = med(cells_written(mk, 4096, poses(4096, 24, rot0=176.0, step=1.0))[1:])
    res["cells_per_frame_4096"] = 16384
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
