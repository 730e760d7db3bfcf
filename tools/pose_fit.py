"""Camera pose refinement through the ray gradients (autograd.radiance_rays in origins and dirs).  Needs the GPU.

    python tools/pose_fit.py [--side 64] [--steps 200] [--offset 0.02] [--angle 0.5] [--lr-t 2e-3] [--lr-w 1e-3] [--decay 0.985] [--out FILE]

A pinhole camera at (0, 0, -1) looks along +z at the `-g 16` scene (256 Gaussians on the plane z = 1) with side x side rays over the
grid's extent.  The pose is six parameters: a translation t of the camera's origin and a rotation vector w (Rodrigues) of its rays, both
0 at the true pose.  The rays are built from them with torch ops; the target is the radiance bundle of the true pose; the fit starts
`--offset` units (along (1, -1, 0.5) normalised) and `--angle` degrees (about (1, 2, 0.5) normalised) off and runs `--steps` steps of
Adam on sum (L - L*)^2, both learning rates falling by `--decay` per step.  No parameter of the scene requires grad, so every backward
passes no table: ray rows only, no atomic add.
Prints the loss and the host time of every step (forward, backward and update, the device waited for), then one JSON line with the
loss curve, the median step time and the pose error at the start and at the end; `--out` writes that line to a file as well.  Fails
unless the loss has fallen to a thousandth and both pose errors to a quarter of where they started.  (The scene is a plane seen head-on:
a sideways shift d and a yaw of d / 2 radians move its image alike to first order, so the fit comes down that valley slowly -- the
last seventh of offset and angle, 0.0027 units against 0.072 degrees, is still there after 200 steps.)
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
from sgrt_amd import autograd, scene  # noqa: E402


def rotation(w):
    import torch
    th = torch.linalg.norm(w) + 1e-20
    zero = torch.zeros((), device=w.device)
    Kx = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
    return torch.eye(3, device=w.device) + torch.sin(th) / th * Kx + (1 - torch.cos(th)) / th ** 2 * (Kx @ Kx)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--offset", type=float, default=0.02)
    ap.add_argument("--angle", type=float, default=0.5)
    ap.add_argument("--lr-t", type=float, default=2e-3)
    ap.add_argument("--lr-w", type=float, default=1e-3)
    ap.add_argument("--decay", type=float, default=0.985)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    g = scene.grid_scene(16)
    r = pkg.Renderer(0)
    dev = torch.device("cuda", 0)
    ps = [torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)
          for x in (g["mu"][:, :3], g["albedo"], g["sigma"], g["magnitude"])]
    u = (np.arange(a.side) + 0.5) / a.side - 0.5
    x, y = np.meshgrid(u, u)
    d0 = np.stack([x.ravel(), y.ravel(), np.ones(a.side * a.side)], 1)       # the grid spans [-1, 1] two units ahead
    d0 = torch.tensor(d0 / np.linalg.norm(d0, axis=1, keepdims=True), dtype=torch.float32, device=dev)
    o0 = torch.tensor([0.0, 0.0, -1.0], device=dev)

    def radiance(t, w):
        dirs = torch.nn.functional.normalize(d0 @ rotation(w).T, dim=1)
        return autograd.radiance_rays(r, *ps, o0 + t, dirs)
    zero = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = radiance(zero, zero + 1e-12)
    t_dir, w_dir = np.array([1.0, -1.0, 0.5]), np.array([1.0, 2.0, 0.5])
    t = torch.tensor(a.offset * t_dir / np.linalg.norm(t_dir), dtype=torch.float32, device=dev, requires_grad=True)
    w = torch.tensor(np.deg2rad(a.angle) * w_dir / np.linalg.norm(w_dir), dtype=torch.float32, device=dev, requires_grad=True)
    opt = torch.optim.Adam([{"params": [t], "lr": a.lr_t}, {"params": [w], "lr": a.lr_w}])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, a.decay)
    start = (float(t.norm()), float(np.rad2deg(w.norm().item())))
    losses, ms = [], []
    for step in range(a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = ((radiance(t, w) - target) ** 2).sum()
        loss.backward()
        opt.step()
        sched.step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        losses.append(loss.item())
        print(f"step {step:3d}  loss {losses[-1]:.6e}  {ms[-1]:.2f} ms")
    with torch.no_grad():
        losses.append(((radiance(t, w) - target) ** 2).sum().item())
    end = (float(t.norm()), float(np.rad2deg(w.norm().item())))
    r.close()
    res = {"what": "tools/pose_fit.py: a pinhole camera's six pose parameters recovered through the ray gradients, table off", "scene": "-g 16",
           "rays": a.side * a.side, "steps": a.steps, "lr_t": a.lr_t, "lr_w": a.lr_w, "decay": a.decay, "loss": [float(f"{v:.6e}") for v in losses],
           "step_ms_median": round(float(np.median(ms[1:])), 3), "step_ms_min": round(float(np.min(ms[1:])), 3),
           "offset_start": start[0], "offset_end": end[0], "angle_deg_start": start[1], "angle_deg_end": end[1]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    assert losses[-1] <= 1e-3 * losses[0], "the loss has to fall to a thousandth of its start"
    assert end[0] <= 0.25 * start[0] and end[1] <= 0.25 * start[1], "the pose has to come within a quarter of where it started"


if __name__ == "__main__":
    main()
