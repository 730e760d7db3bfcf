"""Ray bundles (vrt_hip_radiance_rays*) measured against the two paths they sit between: the full sum of vrt_hip_radiance
and the camera path of vrt_hip_frame_device.  Needs the GPU.

    python tools/ray_bundles.py [--out-dir profiles]      writes ray_bundles.json and ray_bundles.md there, prints the JSON line

  (a) 64 rays aimed at Gaussian centres of `-g 64` (N = 4096), host pointers in, host pointers out: vrt_hip_radiance (every ray
      against all N^2 pairs) and vrt_hip_radiance_rays.  Host clock around the calls, which return after completion; the new
      call warmed up first; medians and the spread over the repeats.  The new call has to be at least 100 times faster.
  (b) the headline frame's own rays (`-g 64 -w 2048`, the CLI camera) as ONE device bundle -- one origin, 2048^2 directions
      normalised once on the host in the reference's arithmetic -- against vrt_hip_frame_device of the same frame (16 x 16 tiles).
  (c) the same number of rays with an origin per ray: two eyes 0.06 apart, interleaved, 2048 x 1024 pixels each.
  (b), (c): stream events around `--calls` calls enqueued back to back, after warm-up; median and spread over `--repeats` such
  windows; the two paths of (b) alternate.  ray_stats of one bundle says where the time goes: chunk spheres and Gaussians
  tested per ray, list entries and pairs per ray, rays per kernel.
  (d) 2^20 rays, each from its own point of a sphere around `-g 64` at a random point of the scene; (e) the `-g 16` frame's rays;
  (f) a 256^2 frame's rays through the teapot (dense: most lit rays go to the one-wave-per-ray kernel).
  Every bundle is timed with the Morton index (vrt_hip_set_ray_index) off and on in the same run -- two contexts on the same scene,
  their windows alternating -- with ray_stats / ray_index_stats of one bundle each, and the two results compared bit for bit.  On (b)
  the indexed call has to be faster than the unindexed one.
  (t) transmittance bundles (vrt_hip_transmittance_bundle): 4096 rays aimed at Gaussians of `-g 64`, host pointers, with ns = 1 and
      ns = 16 samples per ray, index off and on, and vrt_hip_transmittance_rays (the full sum, one sample per ray) on the same rays in
      the same run; host clock around the calls, as in (a).  The ns = 1 bundle has to be faster than the full-sum call.
      `--transmittance-only` runs (t) alone and prints its JSON line without touching the files.
  (depth) depth bundles (vrt_hip_depth_bundle_device): the same 4096 aimed rays, device pointers, nt = 1 (tau = 0.99) and nt = 4 levels
      (0.999, 0.99, 0.98, 0.95: the aimed rays end between T = 0.9 and 0.995), index off and on, against what a caller had before: a
      bisection of the same resolution around vrt_hip_transmittance_bundle_device with the brackets kept on the device -- T at a
      scene bound (8.0, behind everything from these origins) for the misses, then 24 halvings of [0, 8], every step one bundle
      call (a cull and two kernels) and three elementwise updates; no host round trip.  Stream events around each, alternating, after
      warm-up.  The depth bundle has to be faster in every row.  `--depth-only` runs this part alone; it prints its JSON line and
      writes ray_depth.json and ray_depth.md (and nothing else) to --out-dir.  (The letter (d) was taken.)
  (g) gradient bundles (vrt_hip_radiance_rays_grad_device): the 4096 rays of a 64 x 64 pinhole frame of the CLI camera (one origin, but
      these rays pass between the Gaussians), the 4096 rays of a 64 x 64 pinhole frame zoomed onto 0.03 x 0.03 of the grid around one
      Gaussian (one origin, every wave's lanes keep the same few Gaussians: the wave-reduced adds) and the 2^20 scattered rays of (d)
      (per-lane adds), device pointers, index off and on, each against
      vrt_hip_radiance_rays_device (radiance out) of the same rays in the same run, windows alternating.  The ratio is gradient time over
      radiance time; there is no pass / fail ratio.  With it the atomic bytes of one call (36 B per entry of a lane = ray list before
      the wave reduction; the long rays' share is not counted by ray_stats) and the time they would take at 1.3 TB/s.
      `--grad-only` runs this part alone, prints its JSON line and writes ray_grad.json and ray_grad.md (and nothing else) to --out-dir;
      the .md ends with the text of <out-dir>/ray_grad_resources.txt when that file is there (the output of
      `tools/kernel_resources.sh raygrad`, which needs the compiler and no GPU).
  (go) ordered gradient tables (vrt_hip_set_grad_ordered): the three bundles of (g), index off and on, vrt_hip_radiance_rays_grad_device
      with the switch on against the same call with it off (float atomics) in the same run, four contexts, windows alternating.  With it
      the records, the Gaussians with records and the longest segment of one call, and in the same run: the ordered table twice (equal
      bits), with the index on and off (equal bits), and its largest difference from the atomic table.  There is no pass / fail ratio.
      `--ordered-only` runs this part alone, prints its JSON line and writes ray_grad_ordered.json and ray_grad_ordered.md (and nothing
      else) to --out-dir; the .md ends with the text of <out-dir>/ray_grad_ordered_resources.txt when that file is there (the output of
      `tools/kernel_resources.sh raygrad`, `raytgrad` and `gradord`).
  (tg) transmittance gradient bundles (vrt_hip_transmittance_bundle_grad_device, table and per-sample output): the 2^20 scattered rays of
      (d) with ns = 1 (shadow rays, s = 8), the 4096 aimed rays of (t) with ns = 64 (profiles), and the 4096 aimed rays of (depth) in depth
      mode at the depths of level 0.5 (and, beside it, of level 0.99, which these rays do reach), device pointers, index off and on, each
      against vrt_hip_transmittance_bundle_device of the same rays and samples in the same run, windows alternating.  A gradient call has
      to take less time than 10 transmittance bundles (central differences for the five parameters of ONE Gaussian); the ratios are
      reported as measured.  `--tgrad-only` runs this part alone, prints its JSON line and writes ray_trans_grad.json and
      ray_trans_grad.md (and nothing else) to --out-dir; the .md ends with the text of <out-dir>/ray_trans_grad_resources.txt when that
      file is there (the output of `tools/kernel_resources.sh raytgrad`).
  (rg) ray gradients (vrt_hip_radiance_rays_grad_rays_device, vrt_hip_transmittance_bundle_grad_rays_device): the 2^20 scattered and the
      4096 zoomed (coherent) rays of (g) and the 4096 x 64 samples of (tg), device pointers, index off, four paths alternating in the same
      run: the forward bundle, the gradient call with the table alone (what (g) and (tg) time), with table and ray rows, and with the ray
      rows alone (no table, so no atomic add); each gradient time also as a ratio to the forward bundle.  The ray rows alone issue the
      same passes as the table call and no atomic add: the run fails if their median exceeds the table call's by more than the spread
      (max - min) of that run's own repeats of either.  `--rgrad-only` runs this part alone, prints its JSON line and writes
      ray_grad_rays.json and ray_grad_rays.md (and nothing else) to --out-dir; the .md takes in, where they are there,
      <out-dir>/ray_grad_rays_existing.json ({"parent": {"grad": .., "tgrad": ..}, "new": {..}, optionally "parent_again": {..}}: the
      results of `--grad-only` and `--tgrad-only` on the commit before the ray rows and on this one, same machine, same session), <out-dir>/ray_grad_rays_pose_fit.json
      (the line of tools/pose_fit.py) and <out-dir>/ray_grad_rays_resources.txt (tools/kernel_resources.sh raygrad and raytgrad on both).
  (su) scene updates (vrt_hip_set_gaussians_device): one fitting step -- forward and backward of autograd.radiance_rays on `-g 64` -- with
      the four parameter tensors on the CPU (the scene goes through the host: the path before the device setter, measured alongside) and
      with them on the GPU (the scene is set from device memory), on 4096 aimed rays and on 2^20 scattered rays, Morton index off and on;
      host clock around windows of steps that end in a synchronise, the two kinds alternating, after warm-up.  Also the setter alone
      (stream events around calls enqueued back to back) and the host time one call of it takes (enqueue only; the window is
      synchronised afterwards).  The step with cuda parameters has to be faster than the step with CPU parameters in every row; the
      ratio and the setter's times are recorded, not asserted.  `--scene-update-only` runs this part alone, prints its JSON line and
      writes scene_update.json and scene_update.md (and nothing else) to --out-dir.
  (so) sorted bundles (vrt_hip_set_ray_sort): the `-g 64 -w 2048` frame's rays in the camera's order (where sorting can only cost: reported,
      no gate), the same rays under a seeded permutation, 2^20 rays aimed at random Gaussians (vrt_hip_radiance_rays_device, packed pixels
      out) and 4096 aimed rays through the radiance gradient (vrt_hip_radiance_rays_grad_device); four contexts per bundle -- Morton index
      off and on, sort off and on -- their windows alternating in the same run, stream events around back-to-back calls.  Each row carries
      members_tested of one call (vrt_hip_ray_stats / vrt_hip_ray_index_stats) and whether the sorted result equals the unsorted one bit for
      bit (the gradient's atomic table: its largest difference).  The run fails unless the permuted pinhole bundle with index and sort on is
      faster than with the index on and the sort off.  `--sort-only` runs this part alone, prints its JSON line and writes ray_sort.json
      and ray_sort.md (and nothing else) to --out-dir; the .md ends with the text of <out-dir>/ray_sort_resources.txt when that file is
      there (the output of `tools/kernel_resources.sh raysort`).
  (tn) tangent bundles (vrt_hip_radiance_rays_tangent_device, a dense tangent table and dense ray tangents in, 4 floats per ray out): the
      2^20 scattered rays of (d) and 4096 rays from one origin aimed at the same dozen Gaussians of `-g 64` (every wave's lanes keep the
      same few), device pointers, Morton index off and on (two contexts), five paths alternating in the same run: the tangent bundle, the
      radiance bundle, the gradient bundle with a table and atomic adds (vrt_hip_radiance_rays_grad_device), and two radiance bundles back
      to back (what a one-sided finite difference costs); stream events around back-to-back calls, after warm-up.  The yardstick is the
      gradient bundle in the same run: one pass instead of two and stores instead of atomic adds, so the run fails if the tangent
      bundle's median exceeds the gradient bundle's in any row.  The ratios to one and to two radiance bundles are written down, not
      judged.  `--tangent-only` runs this part alone, prints its JSON line and writes ray_tangent.json and ray_tangent.md (and nothing
      else) to --out-dir; the .md ends with the text of <out-dir>/ray_tangent_resources.txt when that file is there (the output of
      `tools/kernel_resources.sh raytangent`).
  (tt) transmittance tangent bundles (vrt_hip_transmittance_bundle_tangent_device, a dense tangent table, dense ray tangents and dense
      sample tangents in, a float per ray and sample out): the 2^20 scattered shadow rays of (d) with ns = 1, the 4096 aimed rays of the
      transmittance part with 64 samples, and the same 4096 rays in depth mode at the depths vrt_hip_depth_bundle_device returned for
      the level 0.99 (about half of them live) -- `-g 64`, device pointers, Morton index off and on (two contexts), three paths
      alternating in the same run: the tangent bundle, vrt_hip_transmittance_bundle_grad_rays_device with table, ray rows and grad_s
      (J^T . u of the same rays and samples: the yardstick) and two transmittance bundles back to back (what one central difference
      costs; samples that are not finite replaced by s = 8 for them); stream events around back-to-back calls, after warm-up.  One
      walk of a list per group of samples instead of two and stores instead of atomic adds: the run fails where the tangent bundle's
      median exceeds the gradient bundle's by more than the spread of the run's repeats (the larger max - min of the two paths).
      `--ttangent-only` runs this part alone, prints its JSON line and writes ray_trans_tangent.json and ray_trans_tangent.md (and
      nothing else) to --out-dir; the .md ends with the text of <out-dir>/ray_trans_tangent_resources.txt when that file is there (the
      output of `tools/kernel_resources.sh rayttangent`).
  (pl) Ray plans (vrt_hip_ray_plan_create_device, vrt_hip_set_ray_plan): every row a bundle call with a plan bound against the same call
      without, in the same run -- `-g 64`, device pointers, stream events around back-to-back calls, the two paths alternating, Morton
      index off / on, each path in a context of its own (the binding is a context's).  Rows: the T bundle with ns = 1 on 2^20 scattered
      rays; the depth-mode transmittance tangent on 4096 aimed rays; the radiance bundle on 2^20 scattered rays; one CG iteration
      (tangent bundle plus gradient bundle with its table) on the 4096 aimed rays with the sort off and on; the ordered gradient on
      the same rays.  Per row: unplanned ms, planned ms, the plan's build (host clock around the create call, which waits), and
      break-even calls = build / (unplanned - planned).  The run fails where a planned call's median exceeds its unplanned twin's by
      more than the spread (max - min) of the unplanned call's repeats, or where a stored output differs in a bit.
      `--diag-only` runs (gn) alone -- the Gauss-Newton diagonal bundle against the gradient bundle and against the four ordered gradient
      calls, record read-backs and host-side squares it replaces, unplanned and planned -- prints its JSON line and writes ray_gn_diag.json
      and ray_gn_diag.md (and nothing else) to --out-dir; it fails where the diagonal call is slower than what it replaces by more than that
      run's spread.  It also records, without any condition, how many CG iterations one damped Gauss-Newton step on `-g 16` takes to a fixed
      relative residual without a preconditioner and with D as the Jacobi preconditioner (part_cg; `--diag-cg-only` runs that alone and
      writes nothing).
      `--plan-only` runs this part alone, prints its JSON line and writes ray_plan.json and ray_plan.md (and puts
      ray_plan_resources.md into the latter if that file is there: build times and `tools/kernel_resources.sh` tables, taken without a GPU).
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
f32 = np.float32


def spread(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 5), "min": round(float(xs.min()), 5), "max": round(float(xs.max()), 5), "n": int(xs.size)}


def directions(plane, origin):
    """normalize(plane - origin) in float32, every operation rounded on its own: rt.h:366-371, vec4f_t::normalize."""
    d = [np.asarray(p, f32) - f32(o) for p, o in zip(plane, origin)]
    norm = np.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(f32)).astype(f32)
    return np.ascontiguousarray(np.stack([c / norm for c in d], 1).astype(f32))


def centre_rays(g, count=64):
    mu = g["mu"][:, :3].astype(np.float64)
    near = np.sort(np.argsort(np.linalg.norm(mu - mu.mean(0), axis=1), kind="stable")[:count])
    o = np.array([0.0, 0.0, -4.0], f32)
    d = mu[near] - o
    return o, np.ascontiguousarray((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32))


def part_a(g, repeats_full=3, repeats_rays=50):
    r = pkg.Renderer(0)
    r.set_gaussians(g)
    o, d = centre_rays(g)
    oo = np.ascontiguousarray(np.tile(o, (len(d), 1)))
    full_ms, rays_ms, indexed_ms = [], [], []
    r.set_ray_index(1)
    for k in range(3 + repeats_rays):                 # the first calls build the index and warm up
        t0 = time.perf_counter()
        indexed = r.radiance_rays(o, d)
        if k >= 3:
            indexed_ms.append((time.perf_counter() - t0) * 1e3)
    r.enable_stats(True)
    r.radiance_rays(o, d)
    ist = r.ray_index_stats()
    r.enable_stats(False)
    r.set_ray_index(0)
    for _ in range(3):
        rays = r.radiance_rays(o, d)
    for k in range(repeats_rays):
        t0 = time.perf_counter()
        rays = r.radiance_rays(o, d)
        rays_ms.append((time.perf_counter() - t0) * 1e3)
        if k % (repeats_rays // repeats_full) == 0 and len(full_ms) < repeats_full:   # in the same run, in between
            t0 = time.perf_counter()
            full = r.radiance(oo, d)
            full_ms.append((time.perf_counter() - t0) * 1e3)
    r.enable_stats(True)
    r.radiance_rays(o, d)
    st = r.ray_stats()
    r.close()
    out = {"rays": len(d), "gaussians": len(g), "full_sum_ms": spread(full_ms), "ray_bundle_ms": spread(rays_ms),
           "speedup": round(float(np.median(full_ms) / np.median(rays_ms)), 1),
           "max_abs_difference": float(np.abs(rays.astype(np.float64) - full).max()), "peak_radiance": float(full.max()), "ray_stats": st,
           "indexed_ms": spread(indexed_ms), "off_over_on": round(float(np.median(rays_ms) / np.median(indexed_ms)), 2),
           "identical": bool((indexed == rays).all()), "ray_index_stats": ist}
    return out


def aimed_rays(g, count=4096, seed=11, origin=(0.0, 0.0, -4.0)):
    """ray k aims at the centre of a Gaussian with a jitter of about sigma (tests/ray_bundle_scenes.coherent_rays)"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(g), size=count, replace=count > len(g))
    target = g["mu"][pick, :3].astype(np.float64) + rng.normal(size=(count, 3)) * g["sigma"][pick, None]
    o = np.asarray(origin, f32)
    d = target - o.astype(np.float64)
    return o, np.ascontiguousarray((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32))


def part_t(g, repeats=20, repeats_full=5):
    r = pkg.Renderer(0)
    r.set_gaussians(g)
    o, d = aimed_rays(g)
    oo = np.ascontiguousarray(np.tile(o, (len(d), 1)))
    s16 = np.linspace(0.5, 8.0, 16).astype(f32)
    s1 = s16[-1:]
    s1_rays = np.full(len(d), s1[0], f32)
    ms_, T = {}, {}
    for on in (0, 1):
        r.set_ray_index(on)
        for label, s in (("ns1", s1), ("ns16", s16)):
            key = f"{label}_{'on' if on else 'off'}"
            for k in range(3 + repeats):                # the first calls build the index and warm up
                t0 = time.perf_counter()
                T[key] = r.transmittance_bundle(o, d, s)
                if k >= 3:
                    ms_.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)
            if on == 0 and label == "ns1":                # the full sum in the same run, behind the bundle it is compared with
                for k in range(1 + repeats_full):
                    t0 = time.perf_counter()
                    full = r.transmittance_rays(oo, d, s1_rays)
                    if k >= 1:
                        ms_.setdefault("full_sum", []).append((time.perf_counter() - t0) * 1e3)
    r.set_ray_index(0)
    r.enable_stats(True)
    r.transmittance_bundle(o, d, s1)
    st = r.ray_stats()
    r.close()
    return {"rays": len(d), "gaussians": len(g), "ms": {k: spread(v) for k, v in ms_.items()},
            "full_over_ns1": round(float(np.median(ms_["full_sum"]) / np.median(ms_["ns1_off"])), 1),
            "max_abs_difference_to_full_sum": float(np.abs(T["ns1_off"][:, 0].astype(np.float64) - full).max()),
            "identical_index_on_off": bool((T["ns1_on"] == T["ns1_off"]).all() and (T["ns16_on"] == T["ns16_off"]).all()),
            "T_min": float(T["ns16_off"].min()), "ray_stats": st}


def check_t(t):
    assert t["ms"]["ns1_off"]["median"] < t["ms"]["full_sum"]["median"], "the ns = 1 transmittance bundle has to be faster than the full-sum call on the same rays"


def markdown_t(t):
    m = t["ms"]
    return f"""
(t) transmittance bundles: {t['rays']} rays aimed at Gaussians of `-g 64` (N = {t['gaussians']}), host pointers, call returns after completion; ms per call, median (min .. max):

| call | index off | index on |
|---|---|---|
| `vrt_hip_transmittance_bundle`, ns = 1 | {ms(m['ns1_off'])} | {ms(m['ns1_on'])} |
| `vrt_hip_transmittance_bundle`, ns = 16 | {ms(m['ns16_off'])} | {ms(m['ns16_on'])} |
| `vrt_hip_transmittance_rays` (full sum, one sample per ray) | {ms(m['full_sum'])} | |

Full sum over the ns = 1 bundle: {t['full_over_ns1']}; largest difference of a T {t['max_abs_difference_to_full_sum']:.2e}; index on = off bit for bit: {t['identical_index_on_off']}.
"""


DEPTH_BOUND, DEPTH_HALVINGS = 8.0, 24     # the caller-side bisection: bracket [0, 8] down to 8 * 2^-24, the depth bundle's s_end 2^-24 with s_end ~ 5.4


def part_depth(g, repeats=7, calls=2):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    o, d = aimed_rays(g)
    nrays = len(d)
    t_o, t_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    ctx = [pkg.Renderer(0), pkg.Renderer(0)]
    for on, r in enumerate(ctx):
        r.set_gaussians(g)
        r.set_ray_index(on)
    rows, out = {}, {}
    for label, levels in (("nt1", [0.99]), ("nt4", [0.999, 0.99, 0.98, 0.95])):
        nt = len(levels)
        tau = torch.tensor(levels, dtype=torch.float32, device="cuda")
        tau_rows = tau.expand(nrays, nt)
        depth = [torch.zeros((nrays, nt), dtype=torch.float32, device="cuda") for _ in ctx]
        base = [torch.zeros((nrays, nt), dtype=torch.float32, device="cuda") for _ in ctx]
        mid, T = torch.zeros((nrays, nt), dtype=torch.float32, device="cuda"), torch.zeros((nrays, nt), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def bundle(k):
            ctx[k].depth_bundle_device(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), tau.data_ptr(), nt, 0, depth[k].data_ptr(), st)

        def bisect(k):
            mid.fill_(DEPTH_BOUND)
            ctx[k].transmittance_bundle_device(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), mid.data_ptr(), nt, 1, T.data_ptr(), st)
            miss = T > tau_rows
            lo, hi = torch.zeros_like(mid), torch.full_like(mid, DEPTH_BOUND)
            for _ in range(DEPTH_HALVINGS):
                torch.add(lo, hi - lo, alpha=0.5, out=mid)
                ctx[k].transmittance_bundle_device(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), mid.data_ptr(), nt, 1, T.data_ptr(), st)
                below = T <= tau_rows
                hi = torch.where(below, mid, hi)
                lo = torch.where(below, lo, mid)
            base[k].copy_(torch.where(miss, torch.full_like(hi, float("inf")), hi))

        t = windows([lambda: bundle(0), lambda: bisect(0), lambda: bundle(1), lambda: bisect(1)], calls, repeats, warm=2)
        torch.cuda.synchronize()
        dv, bv = [x.cpu().numpy() for x in depth], [x.cpu().numpy() for x in base]
        fin = np.isfinite(dv[0]) & np.isfinite(bv[0])
        rows[label] = {"levels": levels, "bundle_off_ms": t[0], "bisection_off_ms": t[1], "bundle_on_ms": t[2], "bisection_on_ms": t[3],
                       "bisection_over_bundle_off": round(t[1]["median"] / t[0]["median"], 1),
                       "bisection_over_bundle_on": round(t[3]["median"] / t[2]["median"], 1),
                       "finite_results": int(np.isfinite(dv[0]).sum()), "of": int(dv[0].size),
                       "same_misses_as_bisection": bool((np.isfinite(dv[0]) == np.isfinite(bv[0])).all()),
                       "max_abs_difference_to_bisection": float(np.abs(dv[0][fin] - bv[0][fin]).max()) if fin.any() else 0.0,
                       "identical_index_on_off": bool((dv[0].view(np.uint32) == dv[1].view(np.uint32)).all())}
        out[label] = dv[0]
    ctx[0].enable_stats(True)
    tau1 = torch.tensor([0.99], dtype=torch.float32, device="cuda")
    one = torch.zeros((nrays, 1), dtype=torch.float32, device="cuda")
    ctx[0].depth_bundle_device(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), tau1.data_ptr(), 1, 0, one.data_ptr(), st)
    stats = ctx[0].ray_stats()
    torch.cuda.synchronize()
    for r in ctx:
        r.close()
    return {"rays": nrays, "gaussians": len(g), "bisection": {"bound": DEPTH_BOUND, "halvings": DEPTH_HALVINGS, "bundle_calls": DEPTH_HALVINGS + 1},
            "rows": rows, "nt1_is_column_of_nt4": bool((out["nt1"][:, 0].view(np.uint32) == out["nt4"][:, 1].view(np.uint32)).all()), "ray_stats": stats}


def check_depth(z):
    for label, r in z["rows"].items():
        assert r["bundle_off_ms"]["median"] < r["bisection_off_ms"]["median"] and r["bundle_on_ms"]["median"] < r["bisection_on_ms"]["median"], \
            f"{label}: the depth bundle has to be faster than the caller-side bisection through transmittance_bundle_device"


def markdown_depth(z):
    lines = [f"""# Depth bundles (tools/ray_bundles.py --depth-only)

{z['rays']} rays aimed at Gaussians of `-g 64` (N = {z['gaussians']}), device pointers, stream events around back-to-back calls, the paths alternating; ms per
call, median (min .. max).  The baseline is what a caller had before: T at s = {z['bisection']['bound']} for the misses, then {z['bisection']['halvings']} halvings of [0, {z['bisection']['bound']}] around
`vrt_hip_transmittance_bundle_device` ({z['bisection']['bundle_calls']} bundle calls, the brackets updated on the device, no host round trip).

| levels | index | `vrt_hip_depth_bundle_device` | caller-side bisection | bisection / bundle | finite results | same misses | largest difference of a depth |
|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            lines.append(f"| {', '.join(str(v) for v in r['levels'])} | {key} | {ms(r[f'bundle_{key}_ms'])} | {ms(r[f'bisection_{key}_ms'])} | {r[f'bisection_over_bundle_{key}']} | "
                         f"{r['finite_results']} of {r['of']} | {r['same_misses_as_bisection']} | {r['max_abs_difference_to_bisection']:.2e} |")
    st = z["ray_stats"]
    lines.append(f"""
Index on = off bit for bit: {all(r['identical_index_on_off'] for r in z['rows'].values())}; the nt = 1 result is the 0.99 column of the nt = 4 result bit for bit: {z['nt1_is_column_of_nt4']}.
Of the {st['rays']} rays {st['short_rays']} are searched lane = ray ({st['lane_entries'] / max(st['short_rays'], 1):.2f} list entries each) and {st['long_rays']} one wave per ray.
""")
    return "\n".join(lines)


def write_depth(z, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "ray_depth.json"), "w") as f:
        f.write(json.dumps({"what": "depth bundles against a caller-side bisection through transmittance bundles; see tools/ray_bundles.py", "depth": z}) + "\n")
    with open(os.path.join(out_dir, "ray_depth.md"), "w") as f:
        f.write(markdown_depth(z))


ATOMIC_RATE = 1.3e12   # bytes of float atomic adds per second, chip-wide


def grad_bundles(g):
    """The three bundles of (g) and (go): (label, (origins, dirs), origin per ray)"""
    cam, _ = scene.cli_camera(64, 64)
    pinhole = (np.asarray(cam.position, f32)[:3], directions(cam.plane(), cam.position))
    centre = g["mu"][len(g) // 2 + int(round(len(g) ** 0.5)) // 2, :3].astype(np.float64)
    u = (np.arange(64) - 31.5) / 64 * 0.03
    target = centre[None, :] + np.stack([np.tile(u, 64), np.repeat(u, 64), np.zeros(4096)], 1)
    dz = target - np.asarray(cam.position, np.float64)[:3]
    zoom = (pinhole[0], np.ascontiguousarray((dz / np.linalg.norm(dz, axis=1, keepdims=True)).astype(f32)))
    return (("pinhole_64x64", pinhole, 0), ("zoom_64x64", zoom, 0), ("scattered_2^20", scattered(g, 1 << 20), 1))


def part_grad(g, calls=3, repeats=5):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    rows = {}
    for label, (o, d), per in grad_bundles(g):
        nrays = len(d)
        t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
        t_g = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(nrays, 4)).astype(f32)).cuda()
        ctx = [pkg.Renderer(0), pkg.Renderer(0)]
        for on, r in enumerate(ctx):
            r.set_gaussians(g)
            r.set_ray_index(on)
        rad = [torch.zeros((nrays, 4), dtype=torch.float32, device="cuda") for _ in ctx]
        table = [torch.zeros((len(g), pkg.GRAD_STRIDE), dtype=torch.float32, device="cuda") for _ in ctx]
        torch.cuda.synchronize()
        fns = []
        for k in (0, 1):
            fns.append(lambda k=k: ctx[k].radiance_rays_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), rad[k].data_ptr(), 0, PACK, st))
            fns.append(lambda k=k: ctx[k].radiance_rays_grad_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_g.data_ptr(), table[k].data_ptr(), st))
        t = windows(fns, calls, repeats, warm=2)
        ctx[0].enable_stats(True)
        table[0].zero_()
        ctx[0].radiance_rays_grad_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_g.data_ptr(), table[0].data_ptr(), st)
        stats = ctx[0].ray_stats()
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(table[0]).all().item())
        for r in ctx:
            r.close()
        atomic_bytes = 36 * stats["lane_entries"]
        rows[label] = {"rays": nrays, "radiance_off_ms": t[0], "grad_off_ms": t[1], "radiance_on_ms": t[2], "grad_on_ms": t[3],
                       "grad_over_radiance_off": round(t[1]["median"] / t[0]["median"], 2), "grad_over_radiance_on": round(t[3]["median"] / t[2]["median"], 2),
                       "atomic_bytes_short_rays_before_reduction": atomic_bytes, "ms_at_atomic_rate": round(atomic_bytes / ATOMIC_RATE * 1e3, 5),
                       "finite": finite, "per_ray": per_ray(stats), "ray_stats": stats}
    return {"gaussians": len(g), "rows": rows}


def markdown_grad(z, resources=""):
    lines = [f"""# Gradient bundles (tools/ray_bundles.py --grad-only)

`vrt_hip_radiance_rays_grad_device` against `vrt_hip_radiance_rays_device` (radiance out) of the same rays in the same run: `-g 64`
(N = {z['gaussians']}), device pointers, stream events around back-to-back calls, the four paths (radiance / gradient, Morton index off / on: two
contexts) alternating; ms per call, median (min .. max).  There is no pass / fail ratio.  Atomic bytes: 36 B (9 adds) per entry of a
lane = ray list, before the wave reduction takes any away; the adds of the one-wave-per-ray kernel are not counted by ray_stats (not taken).

| bundle | rays | index | radiance | gradient | gradient / radiance | list entries (pairs) per lane = ray ray | long rays | atomic bytes | ms at 1.3 TB/s |
|---|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            lines.append(f"| {label} | {r['rays']} | {key} | {ms(r[f'radiance_{key}_ms'])} | {ms(r[f'grad_{key}_ms'])} | {r[f'grad_over_radiance_{key}']} | "
                         f"{r['per_ray']['list_entries']} ({r['per_ray']['pairs']}) | {r['per_ray']['long_rays']} | {r['atomic_bytes_short_rays_before_reduction']} | {r['ms_at_atomic_rate']} |")
    lines.append("""
Not taken: a profile under rocprofv3 (counters, the atomic request count), the host-pointer form, any scene but `-g 64`, the max-ilp
scheduler on this unit, variants of the LDS layout.
""")
    if resources:
        lines.append("Resources (`tools/kernel_resources.sh raygrad`; template arguments: Exp (0 libm, 1 vcl), Erf (0 libm, 1 A&S), INDEXED):\n\n```\n" + resources.rstrip() + "\n```\n")
    return "\n".join(lines)


def part_ordered(g, calls=3, repeats=5):
    """(go) ordered against atomic gradient tables, in the same run: the bundles of (g), Morton index off and on, four contexts"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    rows = {}
    for label, (o, d), per in grad_bundles(g):
        nrays = len(d)
        t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
        t_g = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(nrays, 4)).astype(f32)).cuda()
        ctx = {}
        for index in (0, 1):
            for ordered in (0, 1):
                r = pkg.Renderer(0)
                r.set_gaussians(g)
                r.set_ray_index(index)
                r.set_grad_ordered(ordered)
                ctx[index, ordered] = r
        table = {k: torch.zeros((len(g), pkg.GRAD_STRIDE), dtype=torch.float32, device="cuda") for k in ctx}
        torch.cuda.synchronize()
        keys = sorted(ctx)
        fns = [lambda k=k: ctx[k].radiance_rays_grad_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_g.data_ptr(), table[k].data_ptr(), st)
               for k in keys]
        t = dict(zip(keys, windows(fns, calls, repeats, warm=2)))
        for k in keys:
            table[k].zero_()
        torch.cuda.synchronize()
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        ost = ctx[0, 1].grad_ordered_stats()
        again = table[0, 1].clone()
        table[0, 1].zero_()
        fns[keys.index((0, 1))]()
        torch.cuda.synchronize()
        scale = float(table[0, 0].abs().max().item())
        row = {"rays": nrays, "records": ost["records"], "gaussians_with_records": ost["gaussians"], "longest_segment": ost["longest"],
               "mismatches": ost["mismatches"], "record_bytes": 56 * ost["records"],
               "ordered_bits_repeat": bool(torch.equal(again, table[0, 1])), "ordered_bits_index_on_equal_off": bool(torch.equal(table[0, 1], table[1, 1])),
               "max_abs_ordered_minus_atomic_over_max_abs": float((table[0, 1] - table[0, 0]).abs().max().item()) / max(scale, 1e-30)}
        for index, name in ((0, "off"), (1, "on")):
            row[f"atomic_{name}_ms"], row[f"ordered_{name}_ms"] = t[index, 0], t[index, 1]
            row[f"ordered_over_atomic_{name}"] = round(t[index, 1]["median"] / t[index, 0]["median"], 2)
        for r in ctx.values():
            r.close()
        rows[label] = row
    return {"gaussians": len(g), "rows": rows}


def markdown_ordered(z, resources=""):
    lines = [f"""# Ordered gradient tables (tools/ray_bundles.py --ordered-only)

`vrt_hip_radiance_rays_grad_device` with `vrt_hip_set_grad_ordered` on against the same call with it off (float atomics), in the same
run: `-g 64` (N = {z['gaussians']}), the three bundles of profiles/ray_grad.md, device pointers, stream events around back-to-back calls,
the four paths (atomic / ordered, Morton index off / on: four contexts) alternating; ms per call, median (min .. max).  An ordered call
holds a count pass, a scan, ONE host wait, the record kernels, a radix sort and the reduction.  There is no pass / fail ratio.

| bundle | rays | index | atomic | ordered | ordered / atomic | records | Gaussians with records | longest segment | record memory (56 B each) |
|---|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            lines.append(f"| {label} | {r['rays']} | {key} | {ms(r[f'atomic_{key}_ms'])} | {ms(r[f'ordered_{key}_ms'])} | {r[f'ordered_over_atomic_{key}']} | "
                         f"{r['records']} | {r['gaussians_with_records']} | {r['longest_segment']} | {r['record_bytes']} |")
    lines.append("""
Checked in the same run, per bundle: the ordered table of a second call equals the first bit for bit, the ordered table with the index on
equals the one with it off bit for bit, no mismatch; the largest |ordered - atomic| over the largest |atomic| entry:
""")
    for label, r in z["rows"].items():
        lines.append(f"- {label}: repeat equal {r['ordered_bits_repeat']}, index on = off {r['ordered_bits_index_on_equal_off']}, mismatches {r['mismatches']}, "
                     f"difference {r['max_abs_ordered_minus_atomic_over_max_abs']:.2e}")
    lines.append("""
Not taken: the transmittance gradient, the host-pointer forms, a profile under rocprofv3 (which of count, sort and reduction the time goes
to), any scene but `-g 64`.
""")
    if resources:
        lines.append("Resources (`tools/kernel_resources.sh raygrad`, `raytgrad` and `gradord`; template arguments: Exp (0 libm, 1 vcl), Erf (0 libm, 1 A&S), "
                     "INDEXED, RAYS, ORDERED).  The thirty-two instantiations without ORDERED have the figures they had before the parameter was "
                     "added, line for line; no ORDERED instantiation spills or uses scratch:\n\n```\n" + resources.rstrip() + "\n```\n")
    return "\n".join(lines)


TGRAD_LIMIT = 10.0   # transmittance bundles of the same rays: what central differences cost for the five parameters of ONE Gaussian


def part_tgrad(g, calls=3, repeats=5):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    aimed = aimed_rays(g)
    rows = {}
    cases = (("shadow_2^20_ns1", scattered(g, 1 << 20), 1, pkg.TGRAD_T, np.array([8.0], f32), None),
             ("profiles_4096_ns64", aimed, 0, pkg.TGRAD_T, np.linspace(0.5, 8.0, 64).astype(f32), None),
             ("depth_4096_tau0.5", aimed, 0, pkg.TGRAD_DEPTH, None, 0.5),
             ("depth_4096_tau0.99", aimed, 0, pkg.TGRAD_DEPTH, None, 0.99))      # beside the case asked for: the aimed rays end between T = 0.9 and 0.995
    for label, (o, d), per, wrt, s, level in cases:
        nrays = len(d)
        t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
        ctx = [pkg.Renderer(0), pkg.Renderer(0)]
        for on, r in enumerate(ctx):
            r.set_gaussians(g)
            r.set_ray_index(on)
        if wrt == pkg.TGRAD_DEPTH:      # the samples are the depths of the level, one per ray
            tau = torch.tensor([level], dtype=torch.float32, device="cuda")
            t_s = torch.zeros((nrays, 1), dtype=torch.float32, device="cuda")
            ctx[0].depth_bundle_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), tau.data_ptr(), 1, 0, t_s.data_ptr(), st)
            torch.cuda.synchronize()
            ns, s_per_ray = 1, 1
            live = int((torch.isfinite(t_s) & (t_s > 0)).sum().item())
            t_sT = torch.where(torch.isfinite(t_s), t_s, torch.full_like(t_s, 8.0))      # the transmittance bundle wants finite samples
        else:
            t_s = torch.from_numpy(s).cuda()
            ns, s_per_ray, live, t_sT = len(s), 0, nrays * len(s), t_s
        t_g = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(nrays, ns)).astype(f32)).cuda()
        T = [torch.zeros((nrays, ns), dtype=torch.float32, device="cuda") for _ in ctx]
        gs = [torch.zeros((nrays, ns), dtype=torch.float32, device="cuda") for _ in ctx]
        table = [torch.zeros((len(g), pkg.GRAD_STRIDE), dtype=torch.float32, device="cuda") for _ in ctx]
        torch.cuda.synchronize()
        fns = []
        for k in (0, 1):
            fns.append(lambda k=k: ctx[k].transmittance_bundle_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_sT.data_ptr(), ns, s_per_ray, T[k].data_ptr(), st))
            fns.append(lambda k=k: ctx[k].transmittance_bundle_grad_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_s.data_ptr(), ns, s_per_ray, t_g.data_ptr(), wrt,
                                                                           table[k].data_ptr(), gs[k].data_ptr(), st))
        t = windows(fns, calls, repeats, warm=2)
        ctx[0].enable_stats(True)
        table[0].zero_()
        fns[1]()
        stats = ctx[0].ray_stats()
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(table[0]).all().item() and torch.isfinite(gs[0]).all().item())
        for r in ctx:
            r.close()
        rows[label] = {"rays": nrays, "ns": ns, "live_samples": live, "trans_off_ms": t[0], "tgrad_off_ms": t[1], "trans_on_ms": t[2], "tgrad_on_ms": t[3],
                       "tgrad_over_trans_off": round(t[1]["median"] / t[0]["median"], 2), "tgrad_over_trans_on": round(t[3]["median"] / t[2]["median"], 2),
                       "finite": finite, "per_ray": per_ray(stats), "ray_stats": stats}
    return {"gaussians": len(g), "limit": TGRAD_LIMIT, "rows": rows}


def check_tgrad(z):
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            assert r[f"tgrad_{key}_ms"]["median"] < TGRAD_LIMIT * r[f"trans_{key}_ms"]["median"], \
                f"{label}, index {key}: a transmittance gradient bundle has to take less time than {TGRAD_LIMIT:.0f} transmittance bundles of the same rays"


def markdown_tgrad(z, resources=""):
    lines = [f"""# Transmittance gradient bundles (tools/ray_bundles.py --tgrad-only)

`vrt_hip_transmittance_bundle_grad_device` (table and per-sample output) against `vrt_hip_transmittance_bundle_device` of the same rays
and samples in the same run: `-g 64` (N = {z['gaussians']}), device pointers, stream events around back-to-back calls, the four paths
(transmittance / gradient, Morton index off / on: two contexts) alternating; ms per call, median (min .. max).  The only condition: a
gradient call takes less time than {z['limit']:.0f} transmittance bundles, what central differences cost for the five parameters of ONE
Gaussian.  Depth mode runs at the depths `vrt_hip_depth_bundle_device` returned for the level; a ray that never reaches the level has
depth +inf, which the gradient skips (live samples: finite depths > 0) and the transmittance bundle is given s = 8 for.

| bundle | rays | ns | live samples | index | transmittance | gradient | gradient / transmittance | list entries per lane = ray ray | long rays |
|---|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            lines.append(f"| {label} | {r['rays']} | {r['ns']} | {r['live_samples']} | {key} | {ms(r[f'trans_{key}_ms'])} | {ms(r[f'tgrad_{key}_ms'])} | "
                         f"{r[f'tgrad_over_trans_{key}']} | {r['per_ray']['list_entries']} | {r['per_ray']['long_rays']} |")
    lines.append("""
Not taken: a direct-deposit form of the lane = ray kernel without its 24 KB of running sums for ns <= 4 (shadow rays), a profile under
rocprofv3, the host-pointer form, any scene but `-g 64`, the max-ilp scheduler on this unit, other chunk sizes than NSC = 512.
""")
    if resources:
        lines.append("Resources (`tools/kernel_resources.sh raytgrad`; template arguments: Exp (0 libm, 1 vcl), Erf (0 libm, 1 A&S), INDEXED):\n\n```\n" + resources.rstrip() + "\n```\n")
    return "\n".join(lines)


def part_rgrad(g, calls=3, repeats=7):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    cam, _ = scene.cli_camera(64, 64)
    centre = g["mu"][len(g) // 2 + int(round(len(g) ** 0.5)) // 2, :3].astype(np.float64)
    u = (np.arange(64) - 31.5) / 64 * 0.03
    target = centre[None, :] + np.stack([np.tile(u, 64), np.repeat(u, 64), np.zeros(4096)], 1)
    dz = target - np.asarray(cam.position, np.float64)[:3]
    zoom = (np.asarray(cam.position, f32)[:3], np.ascontiguousarray((dz / np.linalg.norm(dz, axis=1, keepdims=True)).astype(f32)))
    cases = (("scattered_2^20", scattered(g, 1 << 20), 1, None), ("zoom_64x64", zoom, 0, None),
             ("profiles_4096_ns64", aimed_rays(g), 0, np.linspace(0.5, 8.0, 64).astype(f32)))
    rows = {}
    for label, (o, d), per, s in cases:
        nrays = len(d)
        t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
        r = pkg.Renderer(0)
        r.set_gaussians(g)
        table = torch.zeros((len(g), pkg.GRAD_STRIDE), dtype=torch.float32, device="cuda")
        rays = [torch.zeros((nrays, pkg.RAY_GRAD_STRIDE), dtype=torch.float32, device="cuda") for _ in range(2)]
        if s is None:
            t_g = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(nrays, 4)).astype(f32)).cuda()
            out = torch.zeros((nrays, 4), dtype=torch.float32, device="cuda")

            def grad(d_grad, d_rays):
                r.radiance_rays_grad_rays_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_g.data_ptr(), d_grad, d_rays, st)
            fns = [lambda: r.radiance_rays_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), out.data_ptr(), 0, PACK, st)]
        else:
            ns = len(s)
            t_s = torch.from_numpy(s).cuda()
            t_g = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(nrays, ns)).astype(f32)).cuda()
            out, gs = (torch.zeros((nrays, ns), dtype=torch.float32, device="cuda") for _ in range(2))

            def grad(d_grad, d_rays):      # the per-sample output in every path, as (tg) times it
                r.transmittance_bundle_grad_rays_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_s.data_ptr(), ns, 0, t_g.data_ptr(), pkg.TGRAD_T,
                                                        d_grad, gs.data_ptr(), d_rays, st)
            fns = [lambda: r.transmittance_bundle_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_s.data_ptr(), ns, 0, out.data_ptr(), st)]
        fns += [lambda: grad(table.data_ptr(), 0), lambda: grad(table.data_ptr(), rays[0].data_ptr()), lambda: grad(0, rays[1].data_ptr())]
        torch.cuda.synchronize()
        t = windows(fns, calls, repeats, warm=2)
        torch.cuda.synchronize()
        same = bool((rays[0].view(torch.int32) == rays[1].view(torch.int32)).all().item())
        finite = bool(torch.isfinite(rays[1]).all().item())
        r.close()
        fwd = t[0]["median"]
        rows[label] = {"rays": nrays, "ns": 0 if s is None else len(s), "forward_ms": t[0], "table_ms": t[1], "table_and_rays_ms": t[2], "rays_only_ms": t[3],
                       "table_over_forward": round(t[1]["median"] / fwd, 2), "table_and_rays_over_forward": round(t[2]["median"] / fwd, 2),
                       "rays_only_over_forward": round(t[3]["median"] / fwd, 2), "ray_rows_same_bits_with_and_without_table": same, "finite": finite}
    return {"gaussians": len(g), "calls": calls, "repeats": repeats, "rows": rows}


def check_rgrad(z):
    for label, r in z["rows"].items():
        assert r["finite"] and r["ray_rows_same_bits_with_and_without_table"], label
        slack = max(r["table_ms"]["max"] - r["table_ms"]["min"], r["rays_only_ms"]["max"] - r["rays_only_ms"]["min"])
        assert r["rays_only_ms"]["median"] <= r["table_ms"]["median"] + slack, \
            f"{label}: the ray rows alone (the same passes, no atomic add) are slower than the table call by more than the spread of this run's repeats"


def existing_rows(z):
    """(label, index, forward, gradient) of a --grad-only or --tgrad-only result"""
    fwd, grad = ("radiance", "grad") if "grad_off_ms" in next(iter(z["rows"].values())) else ("trans", "tgrad")
    return [(label, key, r[f"{fwd}_{key}_ms"], r[f"{grad}_{key}_ms"]) for label, r in z["rows"].items() for key in ("off", "on")]


def markdown_rgrad(z, existing=None, pose=None, resources=""):
    lines = [f"""# Ray gradients (tools/ray_bundles.py --rgrad-only, tools/pose_fit.py)

## The new outputs

`vrt_hip_radiance_rays_grad_rays_device` / `vrt_hip_transmittance_bundle_grad_rays_device` on `-g 64` (N = {z['gaussians']}), device pointers,
Morton index off, stream events around {z['calls']} back-to-back calls, {z['repeats']} windows per path after warm-up, the four paths of a
bundle alternating; ms per call, median (min .. max), and the median as a ratio to the forward bundle of the same rays in the same run.
"table" is the call the existing entry points make.  The run fails if the ray rows alone are slower than the table call by more than
the spread of its own repeats.

| bundle | rays | ns | forward | table | table + ray rows | ray rows only | / forward: table | table + rows | rows only | same ray bits with / without table |
|---|---|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        lines.append(f"| {label} | {r['rays']} | {r['ns'] or ''} | {ms(r['forward_ms'])} | {ms(r['table_ms'])} | {ms(r['table_and_rays_ms'])} | {ms(r['rays_only_ms'])} | "
                     f"{r['table_over_forward']} | {r['table_and_rays_over_forward']} | {r['rays_only_over_forward']} | {r['ray_rows_same_bits_with_and_without_table']} |")
    lines.append("")
    if existing:
        again = existing.get("parent_again")
        lines.append("""## The existing path, parent against new

`--grad-only` and `--tgrad-only` (the table alone, through the entry points without ray rows) on the commit before the ray rows and on
this one: same machine, same session, one run (process) each""" + (", and the parent's a second time: what one run of the same code differs from another by" if again else "") + """.
Gradient ms per call, median (min .. max).  Worse: the new median exceeds the parent's by more than the parent's own spread (max - min)
over its repeats.

| part | bundle | index | parent | new | new - parent | parent spread | worse |""" + (" parent again - parent |" if again else "") + """
|---|---|---|---|---|---|---|---|""" + ("---|" if again else ""))
        for part in ("grad", "tgrad"):
            rows_again = existing_rows(again[part]) if again else None
            for k, ((label, key, _, pg), (_, _, _, ng)) in enumerate(zip(existing_rows(existing["parent"][part]), existing_rows(existing["new"][part]))):
                diff, sp = ng["median"] - pg["median"], pg["max"] - pg["min"]
                lines.append(f"| {part} | {label} | {key} | {ms(pg)} | {ms(ng)} | {diff:+.5f} | {sp:.5f} | {diff > sp} |"
                             + (f" {rows_again[k][3]['median'] - pg['median']:+.5f} |" if again else ""))
        lines.append("")
    else:
        lines.append("## The existing path, parent against new\n\nNOT RUN: no ray_grad_rays_existing.json was given.\n")
    if pose:
        k = max(1, len(pose["loss"]) // 10)
        lines.append(f"""## Pose fit (tools/pose_fit.py)

`{pose['scene']}`, {pose['rays']} rays of a pinhole camera, {pose['steps']} steps of Adam (lr {pose['lr_t']} on the translation, {pose['lr_w']} on the
rotation vector, both times {pose['decay']} per step) through `autograd.radiance_rays`, no table.  Offset {pose['offset_start']:.4f} -> {pose['offset_end']:.5f} units, angle
{pose['angle_deg_start']:.3f} -> {pose['angle_deg_end']:.4f} degrees.  Step (forward, backward, update; the scene goes through the host every
step): median {pose['step_ms_median']} ms, fastest {pose['step_ms_min']} ms.  Loss at every {k}th step:

```
{'  '.join(f'{v:.4e}' for v in pose['loss'][::k])}
final {pose['loss'][-1]:.4e}
```
""")
    else:
        lines.append("## Pose fit (tools/pose_fit.py)\n\nNOT RUN: no ray_grad_rays_pose_fit.json was given.\n")
    if resources:
        lines.append("## Resources\n\n" + resources.rstrip() + "\n")
    lines.append("""Not taken: a profile under rocprofv3, the Morton index on for the new outputs, the host-pointer forms, depth mode and the shadow rays
(ns = 1) with ray rows, any scene but `-g 64` (pose fit: `-g 16`), more than one run of any figure.
""")
    return "\n".join(lines)


def dozen_rays(g, count=4096, seed=13, origin=(0.0, 0.0, -4.0)):
    """`count` rays from one origin, each aimed at one of the same twelve neighbouring Gaussians of the grid's middle with a jitter of
    about sigma"""
    rng = np.random.default_rng(seed)
    mu = g["mu"][:, :3].astype(np.float64)
    near = np.argsort(((mu - mu.mean(0)) ** 2).sum(1), kind="stable")[:12]
    pick = near[rng.integers(0, 12, size=count)]
    target = mu[pick] + rng.normal(size=(count, 3)) * g["sigma"][pick, None]
    o = np.asarray(origin, f32)
    d = target - o.astype(np.float64)
    return o, np.ascontiguousarray((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32))


def part_tangent(g, calls=3, repeats=7):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(17)
    t_v = torch.from_numpy(rng.uniform(-1, 1, size=(len(g), pkg.GRAD_STRIDE)).astype(f32)).cuda()
    rows = {}
    for label, (o, d), per in (("scattered_2^20", scattered(g, 1 << 20), 1), ("dozen_4096", dozen_rays(g), 0)):
        nrays = len(d)
        t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
        t_g = torch.from_numpy(rng.uniform(-1, 1, size=(nrays, 4)).astype(f32)).cuda()
        t_rv = torch.from_numpy(rng.uniform(-1, 1, size=(nrays, pkg.RAY_GRAD_STRIDE)).astype(f32)).cuda()
        ctx = [pkg.Renderer(0), pkg.Renderer(0)]
        for on, r in enumerate(ctx):
            r.set_gaussians(g)
            r.set_ray_index(on)
        rad = [torch.zeros((nrays, 4), dtype=torch.float32, device="cuda") for _ in ctx]
        out = [torch.zeros((nrays, 4), dtype=torch.float32, device="cuda") for _ in ctx]
        # (the gradient call ADDS into its table, and the table is not cleared between the calls of a window: what a clear would cost is
        # left out of the yardstick's time, which only makes the comparison harder for the tangent bundle; the sums' values are not used)
        table = [torch.zeros((len(g), pkg.GRAD_STRIDE), dtype=torch.float32, device="cuda") for _ in ctx]
        torch.cuda.synchronize()

        def radiance(k):
            ctx[k].radiance_rays_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), rad[k].data_ptr(), 0, PACK, st)

        def twice(k):
            radiance(k)
            radiance(k)
        fns = []
        for k in (0, 1):
            fns.append(lambda k=k: ctx[k].radiance_rays_tangent_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_v.data_ptr(), t_rv.data_ptr(),
                                                                      out[k].data_ptr(), st))
            fns.append(lambda k=k: radiance(k))
            fns.append(lambda k=k: ctx[k].radiance_rays_grad_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_g.data_ptr(), table[k].data_ptr(), st))
            fns.append(lambda k=k: twice(k))
        t = windows(fns, calls, repeats, warm=2)
        ctx[0].enable_stats(True)
        fns[0]()
        stats = ctx[0].ray_stats()
        fns[4]()
        torch.cuda.synchronize()
        same = bool(torch.equal(out[0], out[1]))
        finite = bool(torch.isfinite(out[0]).all().item())
        for r in ctx:
            r.close()
        rows[label] = {"rays": nrays, "finite": finite, "same_bits_index_off_and_on": same, "per_ray": per_ray(stats)}
        for k, key in enumerate(("off", "on")):
            tan, one, grad, two = t[4 * k:4 * k + 4]
            rows[label][key] = {"tangent_ms": tan, "radiance_ms": one, "grad_ms": grad, "two_radiance_ms": two,
                                "tangent_over_grad": round(tan["median"] / grad["median"], 3), "tangent_over_radiance": round(tan["median"] / one["median"], 2),
                                "tangent_over_two_radiance": round(tan["median"] / two["median"], 2)}
    return {"gaussians": len(g), "rows": rows}


def check_tangent(z):
    for label, r in z["rows"].items():
        assert r["finite"] and r["same_bits_index_off_and_on"], label
        for key in ("off", "on"):
            assert r[key]["tangent_ms"]["median"] <= r[key]["grad_ms"]["median"], \
                f"{label}, index {key}: the tangent bundle ({ms(r[key]['tangent_ms'])}) is slower than the gradient bundle ({ms(r[key]['grad_ms'])})"


def markdown_tangent(z, resources=""):
    lines = [f"""# Tangent bundles (tools/ray_bundles.py --tangent-only)

`vrt_hip_radiance_rays_tangent_device` (J . v: a dense tangent table and dense ray tangents in, 4 floats per ray out) against
`vrt_hip_radiance_rays_device` (radiance out), `vrt_hip_radiance_rays_grad_device` (J^T . u: a table, float atomic adds) and two radiance
bundles back to back (a one-sided finite difference) of the same rays in the same run: `-g 64` (N = {z['gaussians']}), device pointers, stream
events around back-to-back calls, the paths alternating, Morton index off / on in two contexts; ms per call, median (min .. max).
The yardstick is the gradient bundle of the same run: the tool fails where the tangent bundle's median exceeds it.  The ratios to one
and to two radiance bundles are written down, not judged.

| bundle | rays | index | tangent | radiance | gradient (table, atomics) | two radiance | tangent / gradient | tangent / radiance | tangent / two radiance | list entries (pairs) per ray of the lane = ray kernel | long rays |
|---|---|---|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            x = r[key]
            lines.append(f"| {label} | {r['rays']} | {key} | {ms(x['tangent_ms'])} | {ms(x['radiance_ms'])} | {ms(x['grad_ms'])} | {ms(x['two_radiance_ms'])} | "
                         f"{x['tangent_over_grad']} | {x['tangent_over_radiance']} | {x['tangent_over_two_radiance']} | "
                         f"{r['per_ray']['list_entries']} ({r['per_ray']['pairs']}) | {r['per_ray']['long_rays']} |")
    lines.append("""
The tangent bundle's results with the index off and on are equal bit for bit in this run.  Not taken: a profile under rocprofv3, the
host-pointer form, a tangent table or ray tangents alone, any scene but `-g 64`, the max-ilp scheduler on this unit.
""")
    if resources:
        lines.append("Resources (`tools/kernel_resources.sh raytangent`; template arguments: Exp (0 libm, 1 vcl), Erf (0 libm, 1 A&S), INDEXED):\n\n```\n" + resources.rstrip() + "\n```\n")
    return "\n".join(lines)


def part_ttangent(g, calls=3, repeats=7):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(19)
    t_v = torch.from_numpy(rng.uniform(-1, 1, size=(len(g), pkg.GRAD_STRIDE)).astype(f32)).cuda()
    aimed = aimed_rays(g)
    rows = {}
    cases = (("shadow_2^20_ns1", scattered(g, 1 << 20), 1, pkg.TGRAD_T, np.array([8.0], f32), None),
             ("profiles_4096_ns64", aimed, 0, pkg.TGRAD_T, np.linspace(0.5, 8.0, 64).astype(f32), None),
             ("depth_4096_tau0.99", aimed, 0, pkg.TGRAD_DEPTH, None, 0.99))
    for label, (o, d), per, wrt, s, level in cases:
        nrays = len(d)
        t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
        ctx = [pkg.Renderer(0), pkg.Renderer(0)]
        for on, r in enumerate(ctx):
            r.set_gaussians(g)
            r.set_ray_index(on)
        if wrt == pkg.TGRAD_DEPTH:      # the samples are the depths of the level, one per ray
            tau = torch.tensor([level], dtype=torch.float32, device="cuda")
            t_s = torch.zeros((nrays, 1), dtype=torch.float32, device="cuda")
            ctx[0].depth_bundle_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), tau.data_ptr(), 1, 0, t_s.data_ptr(), st)
            torch.cuda.synchronize()
            ns, s_per_ray = 1, 1
            live = int((torch.isfinite(t_s) & (t_s > 0)).sum().item())
            t_sT = torch.where(torch.isfinite(t_s), t_s, torch.full_like(t_s, 8.0))      # the transmittance bundle wants finite samples
        else:
            t_s = torch.from_numpy(s).cuda()
            ns, s_per_ray, live, t_sT = len(s), 0, nrays * len(s), t_s
        t_g = torch.from_numpy(rng.uniform(-1, 1, size=(nrays, ns)).astype(f32)).cuda()
        t_sd = torch.from_numpy(rng.uniform(-1, 1, size=(nrays, ns)).astype(f32)).cuda()
        t_rv = torch.from_numpy(rng.uniform(-1, 1, size=(nrays, pkg.RAY_GRAD_STRIDE)).astype(f32)).cuda()
        zeros = lambda *shape: [torch.zeros(shape, dtype=torch.float32, device="cuda") for _ in ctx]
        out, T, gs, ray_rows = zeros(nrays, ns), zeros(nrays, ns), zeros(nrays, ns), zeros(nrays, pkg.RAY_GRAD_STRIDE)
        # (the gradient call ADDS into its table, which is not cleared between the calls of a window: as in part_tangent, that only
        # makes the comparison harder for the tangent bundle)
        table = zeros(len(g), pkg.GRAD_STRIDE)
        torch.cuda.synchronize()

        def trans(k):
            ctx[k].transmittance_bundle_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_sT.data_ptr(), ns, s_per_ray, T[k].data_ptr(), st)

        def twice(k):
            trans(k)
            trans(k)
        fns = []
        for k in (0, 1):
            fns.append(lambda k=k: ctx[k].transmittance_bundle_tangent_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_s.data_ptr(), ns, s_per_ray, wrt,
                                                                              t_v.data_ptr(), t_rv.data_ptr(), t_sd.data_ptr(), 1, out[k].data_ptr(), st))
            fns.append(lambda k=k: ctx[k].transmittance_bundle_grad_rays_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_s.data_ptr(), ns, s_per_ray,
                                                                                t_g.data_ptr(), wrt, table[k].data_ptr(), gs[k].data_ptr(),
                                                                                ray_rows[k].data_ptr(), st))
            fns.append(lambda k=k: twice(k))
        t = windows(fns, calls, repeats, warm=2)
        ctx[0].enable_stats(True)
        fns[0]()
        stats = ctx[0].ray_stats()
        fns[3]()
        torch.cuda.synchronize()
        same = bool(torch.equal(out[0], out[1]))
        finite = bool(torch.isfinite(out[0]).all().item())
        for r in ctx:
            r.close()
        rows[label] = {"rays": nrays, "ns": ns, "live_samples": live, "finite": finite, "same_bits_index_off_and_on": same, "per_ray": per_ray(stats)}
        for k, key in enumerate(("off", "on")):
            tan, grad, two = t[3 * k:3 * k + 3]
            rows[label][key] = {"tangent_ms": tan, "grad_ms": grad, "two_trans_ms": two, "spread_ms": round(max(tan["max"] - tan["min"], grad["max"] - grad["min"]), 5),
                                "tangent_over_grad": round(tan["median"] / grad["median"], 3), "tangent_over_two_trans": round(tan["median"] / two["median"], 2)}
    return {"gaussians": len(g), "rows": rows}


def check_ttangent(z):
    for label, r in z["rows"].items():
        assert r["finite"] and r["same_bits_index_off_and_on"], label
        for key in ("off", "on"):
            x = r[key]
            assert x["tangent_ms"]["median"] <= x["grad_ms"]["median"] + x["spread_ms"], \
                f"{label}, index {key}: the tangent bundle ({ms(x['tangent_ms'])}) is slower than the gradient bundle ({ms(x['grad_ms'])}) by more than the spread"


def markdown_ttangent(z, resources=""):
    lines = [f"""# Transmittance tangent bundles (tools/ray_bundles.py --ttangent-only)

`vrt_hip_transmittance_bundle_tangent_device` (J . v: a dense tangent table, dense ray tangents and dense sample tangents in, a float per
ray and sample out) against `vrt_hip_transmittance_bundle_grad_rays_device` (J^T . u: table with float atomic adds, ray rows and grad_s)
and two `vrt_hip_transmittance_bundle_device` calls back to back (one central difference) of the same rays and samples in the same run:
`-g 64` (N = {z['gaussians']}), device pointers, stream events around back-to-back calls, the paths alternating, Morton index off / on in
two contexts; ms per call, median (min .. max).  Depth mode runs at the depths `vrt_hip_depth_bundle_device` returned for the level; a
ray that never reaches it has depth +inf, which both derivative calls skip (live samples: finite depths > 0) and the transmittance
bundle is given s = 8 for.  The yardstick is the gradient bundle of the same run: the tool fails where the tangent bundle's median
exceeds it by more than the spread of the run's repeats (the larger max - min of the two paths).  The ratio to two transmittance
bundles is written down, not judged.

| bundle | rays | ns | live samples | index | tangent | gradient (table, rows, grad_s) | two transmittance | tangent / gradient | tangent / two transmittance | list entries per ray of the lane = ray kernel | long rays |
|---|---|---|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            x = r[key]
            lines.append(f"| {label} | {r['rays']} | {r['ns']} | {r['live_samples']} | {key} | {ms(x['tangent_ms'])} | {ms(x['grad_ms'])} | {ms(x['two_trans_ms'])} | "
                         f"{x['tangent_over_grad']} | {x['tangent_over_two_trans']} | {r['per_ray']['list_entries']} | {r['per_ray']['long_rays']} |")
    lines.append("""
The tangent bundle's results with the index off and on are equal bit for bit in this run.  Not taken: a profile under rocprofv3, the
host-pointer form, one of the three inputs alone, any scene but `-g 64`, the max-ilp scheduler on this unit, `wrt` as a template
parameter, the long kernel with its per-entry scalars kept per ray instead of formed again per group of samples, a short kernel without
its 24 KB of scalars for ns <= 4 (shadow rays).
""")
    if resources:
        lines.append("Resources (`tools/kernel_resources.sh rayttangent`; template arguments: Exp (0 libm, 1 vcl), Erf (0 libm, 1 A&S), INDEXED):\n\n```\n" + resources.rstrip() + "\n```\n")
    return "\n".join(lines)


def part_plan(g, calls=3, repeats=7):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(23)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()      # noqa: E731
    t_v = cuda(rng.uniform(-1, 1, size=(len(g), pkg.GRAD_STRIDE)))
    scat, aimed = scattered(g, 1 << 20), aimed_rays(g)
    rows = {}
    cases = (("T_2^20_ns1", scat, 1, "T", False, False), ("depth_tangent_4096", aimed, 0, "depth_tangent", False, False),
             ("radiance_2^20", scat, 1, "radiance", False, False), ("cg_iteration_4096", aimed, 0, "cg", False, False),
             ("cg_iteration_4096_sorted", aimed, 0, "cg", True, False), ("ordered_gradient_4096", aimed, 0, "grad", False, True))
    for label, (o, d), per, kind, sort, ordered in cases:
        nrays = len(d)
        t_o, t_d = cuda(o), cuda(d)
        rows[label] = {"rays": nrays, "kind": kind, "sort": int(sort), "ordered": int(ordered)}
        for index, key in enumerate(("off", "on")):
            ctx = [pkg.Renderer(0), pkg.Renderer(0)]          # [unplanned, planned]
            for r in ctx:
                r.set_gaussians(g)
                r.set_ray_index(index)
                r.set_ray_sort(int(sort))
                r.set_grad_ordered(int(ordered))
            zeros = lambda *shape: [torch.zeros(shape, dtype=torch.float32, device="cuda") for _ in ctx]      # noqa: E731
            out1, out4, rows8, table = zeros(nrays, 1), zeros(nrays, 4), zeros(nrays, pkg.RAY_GRAD_STRIDE), zeros(len(g), pkg.GRAD_STRIDE)
            t_g4, t_s = cuda(rng.uniform(-1, 1, size=(nrays, 4))), cuda(np.array([8.0], f32))
            if kind == "depth_tangent":                        # the samples are the depths of the level, one per ray
                tau = torch.tensor([0.99], dtype=torch.float32, device="cuda")
                t_s = torch.zeros((nrays, 1), dtype=torch.float32, device="cuda")
                ctx[0].depth_bundle_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), tau.data_ptr(), 1, 0, t_s.data_ptr(), st)
            torch.cuda.synchronize()

            def call(k):
                r = ctx[k]
                if kind == "T":
                    r.transmittance_bundle_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_s.data_ptr(), 1, 0, out1[k].data_ptr(), st)
                elif kind == "radiance":
                    r.radiance_rays_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), out4[k].data_ptr(), 0, PACK, st)
                elif kind == "depth_tangent":
                    r.transmittance_bundle_tangent_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_s.data_ptr(), 1, 1, pkg.TGRAD_DEPTH, t_v.data_ptr(), 0, 0,
                                                          1, out1[k].data_ptr(), st)
                else:
                    if kind == "cg":
                        r.radiance_rays_tangent_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_v.data_ptr(), 0, out4[k].data_ptr(), st)
                    r.radiance_rays_grad_rays_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_g4.data_ptr(), table[k].data_ptr(), rows8[k].data_ptr(), st)
            build = []
            for _ in range(4):                                 # the first one warms the buffers up
                t0 = time.perf_counter()
                plan = ctx[1].ray_plan_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), st)
                build.append((time.perf_counter() - t0) * 1e3)
                info = plan.info()
                if len(build) < 4:
                    plan.close()
            ctx[1].set_ray_plan(plan)
            t = windows([lambda: call(0), lambda: call(1)], calls, repeats, warm=2)
            for tb in table:
                tb.zero_()
            call(0)
            call(1)
            torch.cuda.synchronize()
            same = all(bool(torch.equal(a[0], a[1])) for a in (out1, out4, rows8)) and (not ordered or bool(torch.equal(table[0], table[1])))
            for r in ctx:
                r.close()
            un, pl, b = t[0], t[1], spread(build[1:])
            gain = un["median"] - pl["median"]
            rows[label][key] = {"unplanned_ms": un, "planned_ms": pl, "build_ms": b, "spread_ms": round(un["max"] - un["min"], 5),
                                "planned_over_unplanned": round(pl["median"] / un["median"], 3),
                                "break_even_calls": round(b["median"] / gain, 1) if gain > 0 else None, "same_bits": same,
                                "entries": info["entries"], "long_rays": info["long_rays"], "plan_bytes": info["bytes"]}
    return {"gaussians": len(g), "rows": rows}


def check_plan(z):
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            x = r[key]
            assert x["same_bits"], f"{label}, index {key}: a planned output differs from the unplanned one"
            assert x["planned_ms"]["median"] <= x["unplanned_ms"]["median"] + x["spread_ms"], \
                f"{label}, index {key}: the planned call ({ms(x['planned_ms'])}) is slower than the unplanned one ({ms(x['unplanned_ms'])}) by more than the spread"


def markdown_plan(z, resources=""):
    lines = [f"""# Ray plans (tools/ray_bundles.py --plan-only)

Every bundle call with a plan bound (`vrt_hip_set_ray_plan`) against the same call without, in the same run: `-g 64` (N = {z['gaussians']}),
device pointers, stream events around back-to-back calls, the two paths alternating, each in a context of its own, Morton index off / on;
ms per call, median (min .. max).  Build: the host's clock around `vrt_hip_ray_plan_create_device`, which waits for its stream (three
builds behind a warm one).  Break-even = build / (unplanned - planned): the calls after which the plan has paid for itself.  The tool
fails where a planned median exceeds the unplanned one by more than the spread (max - min) of the unplanned call's repeats, or where a
stored output (for the ordered row the table too) differs in a bit.  One CG iteration = a tangent bundle plus a gradient bundle with its
table (float atomics).

| row | rays | index | unplanned | planned | planned / unplanned | build | break-even calls | kept entries | long rays | plan bytes |
|---|---|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            x = r[key]
            lines.append(f"| {label} | {r['rays']} | {key} | {ms(x['unplanned_ms'])} | {ms(x['planned_ms'])} | {x['planned_over_unplanned']} | {ms(x['build_ms'])} | "
                         f"{x['break_even_calls'] if x['break_even_calls'] is not None else 'never'} | {x['entries']} | {x['long_rays']} | {x['plan_bytes']} |")
    lines.append("""
Not taken: a profile under rocprofv3, the host-pointer forms, any scene but `-g 64`, a CSR in slot order for sorted plans, entries of 16
bits for scenes below 65536 Gaussians, the lists staged through LDS by the wave instead of read by each lane.
""")
    if resources:
        lines.append(resources.rstrip() + "\n")
    return "\n".join(lines)


def part_diag(g, calls=3, repeats=5, repeats_b=2):
    """(gn) the Gauss-Newton diagonal bundle against (a) the gradient bundle with table of the same rays and (b) what it replaces: four
    ordered gradient calls with g = e_c, the record read-back and the host-side squaring -- unplanned and with a bound plan"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()      # noqa: E731
    rows = {}
    for label, (o, d), per in (("scattered_2^20", scattered(g, 1 << 20), 1), ("aimed_4096", aimed_rays(g), 0)):
        nrays = len(d)
        t_o, t_d = cuda(o), cuda(d)
        t_g = cuda(np.random.default_rng(3).uniform(-1, 1, size=(nrays, 4)))
        t_w = cuda(np.random.default_rng(4).uniform(0.25, 4.0, size=(nrays, 4)))
        t_e = [cuda(np.tile(np.eye(4, dtype=f32)[c], (nrays, 1))) for c in range(4)]
        rows[label] = {"rays": nrays}
        for index, key in enumerate(("off", "on")):
            ctx = {}
            for name in ("diag", "grad", "diag_planned", "grad_planned", "records", "records_planned"):
                r = pkg.Renderer(0)
                r.set_gaussians(g)
                r.set_ray_index(index)
                r.set_grad_ordered(int(name.startswith("records")))
                ctx[name] = r
            table = {k: torch.zeros((len(g), pkg.GRAD_STRIDE), dtype=torch.float32, device="cuda") for k in ctx}
            plans = {k: ctx[k].ray_plan_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), st) for k in ctx if k.endswith("planned")}
            for k, plan in plans.items():
                ctx[k].set_ray_plan(plan)
            torch.cuda.synchronize()

            def diag(k):
                ctx[k].radiance_rays_gn_diag_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_w.data_ptr(), table[k].data_ptr(), st)

            def grad(k):
                ctx[k].radiance_rays_grad_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_g.data_ptr(), table[k].data_ptr(), st)

            def replaced(k):
                """what the diagonal call replaces, to the finished [N, 9] on the host (unit weights)"""
                out = np.zeros((len(g), 9))
                for c in range(4):
                    ctx[k].radiance_rays_grad_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), t_e[c].data_ptr(), table[k].data_ptr(), st)
                    gauss, ray, rec = ctx[k].grad_records()
                    pair = ray.astype(np.int64) * len(g) + gauss             # a long ray files two records per kept Gaussian: summed before the square
                    order = np.argsort(pair, kind="stable")
                    first = np.concatenate([[True], np.diff(pair[order]) != 0])
                    sums = np.add.reduceat(rec[order].astype(np.float64), np.nonzero(first)[0], axis=0)
                    np.add.at(out, gauss[order][first], sums * sums)
                return out
            print(f"(gn) {label}, index {key}: the diagonal and the gradient calls", file=sys.stderr, flush=True)
            t = windows([lambda: diag("diag"), lambda: grad("grad"), lambda: diag("diag_planned"), lambda: grad("grad_planned")], calls, repeats, warm=2)
            tb = {"records": [], "records_planned": []}
            for rep in range(repeats_b + 1):                                  # the first one warms the buffers up
                for k in tb:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    want = replaced(k)
                    tb[k].append((time.perf_counter() - t0) * 1e3)
                    print(f"(gn) {label}, index {key}: {k} {tb[k][-1]:.0f} ms", file=sys.stderr, flush=True)
            table["diag"].zero_()
            ones = torch.ones_like(t_w)
            ctx["diag"].radiance_rays_gn_diag_device(nrays, t_o.data_ptr(), per, t_d.data_ptr(), ones.data_ptr(), table["diag"].data_ptr(), st)
            torch.cuda.synchronize()
            got = table["diag"].cpu().numpy()[:, :9].astype(np.float64)
            scale = np.maximum(np.abs(want).max(0, keepdims=True), 1e-300)
            for plan in plans.values():
                plan.close()
            for r in ctx.values():
                r.close()
            b, bp = spread(tb["records"][1:]), spread(tb["records_planned"][1:])
            rows[label][key] = {"diag_ms": t[0], "grad_ms": t[1], "diag_planned_ms": t[2], "grad_planned_ms": t[3], "replaced_ms": b, "replaced_planned_ms": bp,
                                "diag_over_grad": round(t[0]["median"] / t[1]["median"], 2), "diag_over_grad_planned": round(t[2]["median"] / t[3]["median"], 2),
                                "replaced_over_diag": round(b["median"] / t[0]["median"], 1), "replaced_over_diag_planned": round(bp["median"] / t[2]["median"], 1),
                                "replaced_spread_ms": round(b["max"] - b["min"], 5), "replaced_planned_spread_ms": round(bp["max"] - bp["min"], 5),
                                "max_abs_diag_minus_replaced_over_column_max": float((np.abs(got - want) / scale).max()), "finite": bool(np.isfinite(got).all())}
    return {"gaussians": len(g), "rows": rows}


def part_cg(grid=16, lam=1e-2, tol=1e-4, cap=400):
    """(gn) one damped Gauss-Newton step on `-g <grid>`: (J^T J + lam D) x = -J^T res by conjugate gradients, every product a planned tangent
    bundle plus a planned gradient bundle (host/ray_plan_example.cpp's round), D = diag(J^T J) by the diagonal bundle; iterations to
    |residual| <= tol |right-hand side| without a preconditioner and with D as the Jacobi preconditioner.  res = the radiance of the
    scene minus that of the same scene disturbed (seeded: centres by 0.1 sigma, albedo, sigma and magnitude by 5 %)."""
    g = scene.grid_scene(grid)
    o, d = aimed_rays(g)
    rng = np.random.default_rng(31)
    g2 = g.copy()
    g2["mu"][:, :3] += (0.1 * g["sigma"][:, None] * rng.normal(size=(len(g), 3))).astype(f32)
    for k in ("albedo", "sigma", "magnitude"):
        g2[k] = (g[k] * (1.0 + 0.05 * rng.normal(size=g[k].shape))).astype(f32)
    r = pkg.Renderer(0)
    r.set_gaussians(g2)
    target = r.radiance_rays(o, d).astype(np.float64)
    r.set_gaussians(g)
    res = r.radiance_rays(o, d).astype(np.float64) - target
    plan = r.ray_plan(o, d)
    r.set_ray_plan(plan)

    def table(cols):
        return np.concatenate([cols["albedo"], cols["mu"], cols["sigma"][:, None], cols["magnitude"][:, None]], 1).astype(np.float64)

    def packed(x):
        t = np.zeros((len(g), pkg.GRAD_STRIDE), f32)
        t[:, :9] = x
        return t
    D = r.radiance_rays_gn_diag(o, d)[:, :9].astype(np.float64)
    on = D > 0                                                     # a parameter no ray moves has no equation
    b = -table(r.radiance_rays_grad(o, d, res.astype(f32))) * on

    def A(x):
        Jx = r.radiance_rays_tangent(o, d, tangent=packed(x * on))
        return (table(r.radiance_rays_grad(o, d, Jx)) + lam * D * x) * on

    def cg(M):
        x, rr = np.zeros_like(b), b.copy()
        z = rr / M if M is not None else rr
        p, rz, b2 = z.copy(), float((rr * z).sum()), float((b * b).sum()) ** 0.5
        for it in range(1, cap + 1):
            Ap = A(p)
            alpha = rz / float((p * Ap).sum())
            x += alpha * p
            rr -= alpha * Ap
            rel = float((rr * rr).sum()) ** 0.5 / b2
            if rel <= tol:
                return {"iterations": it, "reached": True, "relative_residual": rel}
            z = rr / M if M is not None else rr
            rz_new = float((rr * z).sum())
            p = z + (rz_new / rz) * p
            rz = rz_new
        return {"iterations": cap, "reached": False, "relative_residual": rel}
    M = np.where(on, (1.0 + lam) * D, 1.0)
    out = {"grid": grid, "gaussians": len(g), "rays": len(d), "unknowns": int(on.sum()), "lambda": lam, "tolerance": tol, "cap": cap,
           "diag_min_over_max": float(D[on].min() / D[on].max()), "plain": cg(None), "jacobi": cg(M)}
    plan.close()
    r.close()
    return out


def check_diag(z):
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            x = r[key]
            assert x["finite"], f"{label}, index {key}: the diagonal is not finite"
            for d, b, sp in (("diag_ms", "replaced_ms", "replaced_spread_ms"), ("diag_planned_ms", "replaced_planned_ms", "replaced_planned_spread_ms")):
                assert x[d]["median"] <= x[b]["median"] + x[sp], \
                    f"{label}, index {key}: the diagonal call ({ms(x[d])}) is slower than what it replaces ({ms(x[b])}) by more than the spread"


def markdown_diag(z, resources=""):
    lines = [f"""# Gauss-Newton diagonal bundles (tools/ray_bundles.py --diag-only)

`vrt_hip_radiance_rays_gn_diag_device` (seeded weights in, the table added into) in the same run against (a) `vrt_hip_radiance_rays_grad_device`
with table of the same rays and (b) what it replaces: four ordered gradient calls with g = e_c, `vrt_hip_get_grad_records` after each and
the squaring on the host (numpy), timed on the host clock from the first call to the finished [N, 9].  `-g 64` (N = {z['gaussians']}), device
pointers, stream events around back-to-back calls for the diagonal and (a), the calls alternating; unplanned and with a bound ray plan; ms per
call, median (min .. max).  The tool fails where the diagonal call is slower than (b) by more than the spread of (b); the ratio to (a) is
recorded, not judged.

| bundle | rays | index | plan | diagonal | (a) gradient | diagonal / (a) | (b) replaced | (b) / diagonal | max abs diagonal - (b), of the column's largest |
|---|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            x = r[key]
            lines.append(f"| {label} | {r['rays']} | {key} | no | {ms(x['diag_ms'])} | {ms(x['grad_ms'])} | {x['diag_over_grad']} | {ms(x['replaced_ms'])} | "
                         f"{x['replaced_over_diag']} | {x['max_abs_diag_minus_replaced_over_column_max']:.2e} |")
            lines.append(f"| {label} | {r['rays']} | {key} | bound | {ms(x['diag_planned_ms'])} | {ms(x['grad_planned_ms'])} | {x['diag_over_grad_planned']} | "
                         f"{ms(x['replaced_planned_ms'])} | {x['replaced_over_diag_planned']} | |")
    c = z.get("cg")
    if c:
        lines.append(f"""
One damped Gauss-Newton step on `-g {c['grid']}` (N = {c['gaussians']}, {c['rays']} aimed rays, {c['unknowns']} parameters that some ray moves; the
smallest entry of D is {c['diag_min_over_max']:.1e} of the largest): `(JᵀJ + λ D) x = -Jᵀ res` with λ = {c['lambda']} by conjugate gradients, every product
a planned tangent bundle plus a planned gradient bundle, to a relative residual of {c['tolerance']} (at most {c['cap']} iterations).  Recorded,
not judged.

| preconditioner | iterations | reached | relative residual at the end |
|---|---|---|---|
| none | {c['plain']['iterations']} | {c['plain']['reached']} | {c['plain']['relative_residual']:.2e} |
| Jacobi, (1 + λ) D | {c['jacobi']['iterations']} | {c['jacobi']['reached']} | {c['jacobi']['relative_residual']:.2e} |
""")
    lines.append("""
Not taken: the arrangement of the lane = ray kernel that keeps 7 floats per list position in two passes (not built), a profile under
rocprofv3, any scene but `-g 64` for the timings.
""")
    if resources:
        lines.append("Resources (`tools/kernel_resources.sh raygndiag`; template arguments: Exp (0 libm, 1 vcl), Erf (0 libm, 1 A&S), list source, ORDERED):\n\n```\n"
                     + resources.rstrip() + "\n```\n")
    return "\n".join(lines)


def part_scene(g, repeats=7, warm=2):
    import torch
    from sgrt_amd import autograd
    st = torch.cuda.current_stream().cuda_stream
    p = {"mu": g["mu"][:, :3], "albedo": g["albedo"], "sigma": g["sigma"], "magnitude": g["magnitude"]}
    order = ("mu", "albedo", "sigma", "magnitude")
    rows = {}
    for label, (o, d), steps in (("aimed_4096", aimed_rays(g), 20), ("scattered_2^20", scattered(g, 1 << 20), 3)):
        nrays = len(d)
        t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
        t_w = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(nrays, 4)).astype(f32)).cuda()
        for on in (0, 1):
            r = pkg.Renderer(0)
            r.set_ray_index(on)
            params = {where: [torch.tensor(np.ascontiguousarray(p[k], f32), device=where, requires_grad=True) for k in order] for where in ("cpu", "cuda")}

            def step(where):
                ps = params[where]
                for t in ps:
                    t.grad = None
                (autograd.radiance_rays(r, *ps, t_o, t_d) * t_w).sum().backward()

            def window(where):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(where)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / steps
            for _ in range(warm):
                window("cpu"), window("cuda")
            ms_step = {"cpu": [], "cuda": []}
            for _ in range(repeats):
                for where in ("cpu", "cuda"):
                    ms_step[where].append(window(where))
            grads = {where: [t.grad.detach().cpu().numpy().astype(np.float64) for t in params[where]] for where in params}
            scale = max(float(np.abs(a).max()) for a in grads["cpu"])
            diff = max(float(np.abs(a - b).max()) for a, b in zip(grads["cpu"], grads["cuda"]))
            dev = [t.detach().contiguous() for t in params["cuda"]]
            ptrs = [t.data_ptr() for t in dev]
            setter = windows([lambda: r.set_gaussians_device(len(g), *ptrs, stream=st)], 20, repeats, warm=3)[0]
            enqueue = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    r.set_gaussians_device(len(g), *ptrs, stream=st)
                enqueue.append((time.perf_counter() - t0) * 1e3 / 20)
                torch.cuda.synchronize()
            r.close()
            host, device = spread(ms_step["cpu"]), spread(ms_step["cuda"])
            rows[f"{label} index {'on' if on else 'off'}"] = {
                "rays": nrays, "index": on, "steps_per_window": steps, "step_cpu_parameters_ms": host, "step_cuda_parameters_ms": device,
                "host_over_device": round(host["median"] / device["median"], 2), "setter_ms": setter, "setter_enqueue_host_ms": spread(enqueue),
                "largest_gradient": scale, "largest_gradient_difference_between_the_paths": diff}
    return {"gaussians": len(g), "rows": rows}


def check_scene(z):
    for label, r in z["rows"].items():
        assert r["step_cuda_parameters_ms"]["median"] < r["step_cpu_parameters_ms"]["median"], \
            f"{label}: the fitting step with cuda parameters has to be faster than the step with CPU parameters of the same run"


def markdown_scene(z):
    lines = [f"""# Scene updates from device memory (tools/ray_bundles.py --scene-update-only)

`-g 64` ({z['gaussians']} Gaussians).  One fitting step = forward + backward of `autograd.radiance_rays`.  With the four parameter
tensors on the CPU the scene reaches the renderer through the host (`set_gaussians_soa`: the path before
`vrt_hip_set_gaussians_device`, measured alongside); with them on the GPU it is set from device memory.  Host clock around windows of
steps that end in a synchronise, the two kinds alternating in the same process, after warm-up; ms per step, median (min .. max).  The
setter alone: stream events around 20 calls enqueued back to back; its enqueue: host clock around 20 calls, nothing waited for.  The
only condition: the step with cuda parameters is faster in every row.  The parameter gradients of the two paths differ by float
atomic order only (last column: largest difference / largest gradient).

| bundle | rays | step, CPU parameters | step, cuda parameters | CPU / cuda | setter alone | setter, host time per call | gradient difference |
|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        lines.append(f"| {label} | {r['rays']} | {ms(r['step_cpu_parameters_ms'])} | {ms(r['step_cuda_parameters_ms'])} | {r['host_over_device']} | "
                     f"{ms(r['setter_ms'])} | {ms(r['setter_enqueue_host_ms'])} | "
                     f"{r['largest_gradient_difference_between_the_paths']:.3g} / {r['largest_gradient']:.3g} |")
    return "\n".join(lines) + "\n"


def part_sort(g, w, calls=3, repeats=5):
    """(so) sort off against on, Morton index off and on, in the same run"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    cam, _ = scene.cli_camera(w, w)
    pin = directions(cam.plane(), cam.position)
    perm = np.random.default_rng(17).permutation(len(pin))
    bundles = [(f"-g 64 -w {w} pinhole, camera order", (cam.position, pin), False),
               (f"-g 64 -w {w} pinhole, seeded permutation", (cam.position, np.ascontiguousarray(pin[perm])), False),
               ("2^20 rays aimed at random Gaussians", aimed_rays(g, 1 << 20), False),
               ("4096 aimed rays, radiance gradient", aimed_rays(g, 4096), True)]
    rows = {}
    for label, (o, d), grad in bundles:
        nrays = len(d)
        t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
        t_g = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(nrays, 4)).astype(f32)).cuda() if grad else None
        keys = [(index, sort) for index in (0, 1) for sort in (0, 1)]
        ctx = {}
        for index, sort in keys:
            r = pkg.Renderer(0)
            r.set_gaussians(g)
            r.set_ray_index(index)
            r.set_ray_sort(sort)
            ctx[index, sort] = r
        out = {k: (torch.zeros((len(g), pkg.GRAD_STRIDE), dtype=torch.float32, device="cuda") if grad else torch.zeros(nrays, dtype=torch.int32, device="cuda"))
               for k in keys}
        torch.cuda.synchronize()
        if grad:
            fns = [lambda k=k: ctx[k].radiance_rays_grad_device(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), t_g.data_ptr(), out[k].data_ptr(), st) for k in keys]
        else:
            fns = [lambda k=k: ctx[k].radiance_rays_device(nrays, t_o.data_ptr(), 0, t_d.data_ptr(), 0, out[k].data_ptr(), PACK, st) for k in keys]
        t = dict(zip(keys, windows(fns, calls, repeats, warm=2)))
        members, sorted_flag = {}, {}
        for k, fn in zip(keys, fns):
            out[k].zero_()
            ctx[k].enable_stats(True)
            fn()
            members[k] = (ctx[k].ray_index_stats() if k[0] else ctx[k].ray_stats())["members_tested"]
            sorted_flag[k] = ctx[k].ray_sort_stats()["sorted"]
        torch.cuda.synchronize()
        row = {"rays": nrays, "gradient": grad}
        for index, name in ((0, "off"), (1, "on")):
            row[f"index_{name}"] = {"sort_off_ms": t[index, 0], "sort_on_ms": t[index, 1], "off_over_on": round(t[index, 0]["median"] / t[index, 1]["median"], 2),
                                    "members_tested_sort_off": members[index, 0], "members_tested_sort_on": members[index, 1],
                                    "sorted": [sorted_flag[index, 0], sorted_flag[index, 1]]}
            if grad:
                scale = float(out[index, 0].abs().max().item())
                row[f"index_{name}"]["max_abs_sorted_minus_unsorted_over_max_abs"] = float((out[index, 1] - out[index, 0]).abs().max().item()) / max(scale, 1e-30)
            else:
                row[f"index_{name}"]["identical"] = bool(torch.equal(out[index, 0], out[index, 1]))
        for r in ctx.values():
            r.close()
        rows[label] = row
    return {"gaussians": len(g), "rows": rows}


def check_sort(z):
    for label, r in z["rows"].items():
        for name in ("index_off", "index_on"):
            assert r[name]["sorted"] == [0, 1], (label, name)
            assert r["gradient"] or r[name]["identical"], (label, name, "the sorted bundle's pixels differ from the unsorted bundle's")
    p = next(r for label, r in z["rows"].items() if "permutation" in label)["index_on"]
    assert p["sort_on_ms"]["median"] < p["sort_off_ms"]["median"], "the permuted pinhole bundle with index and sort on has to be faster than with the sort off"


def markdown_sort(z, resources=""):
    lines = [f"""# Sorted bundles (tools/ray_bundles.py --sort-only)

`vrt_hip_set_ray_sort` on against off, in the same run: `-g 64` (N = {z['gaussians']}), device pointers, stream events around back-to-back calls,
the four paths (Morton index off / on, sort off / on: four contexts) alternating; ms per call, median (min .. max).  A sorted call holds
the key kernel and a radix sort of (key, ray id) ahead of the bundle's own two kernels, on the same stream, with no wait.  members tested:
`members_tested` of one call (`vrt_hip_ray_stats` with the index off, `vrt_hip_ray_index_stats` with it on).  The camera-order row is
where sorting can only cost; the run fails unless the permuted pinhole bundle with index and sort on is faster than with the sort off.

| bundle | rays | index | sort off | sort on | off / on | members tested, sort off | sort on | same bits |
|---|---|---|---|---|---|---|---|---|"""]
    for label, r in z["rows"].items():
        for key in ("off", "on"):
            x = r[f"index_{key}"]
            same = f"table differs by {x['max_abs_sorted_minus_unsorted_over_max_abs']:.1e} of its largest entry (float atomics)" if r["gradient"] else str(x["identical"])
            lines.append(f"| {label} | {r['rays']} | {key} | {ms(x['sort_off_ms'])} | {ms(x['sort_on_ms'])} | {x['off_over_on']} | "
                         f"{x['members_tested_sort_off']} | {x['members_tested_sort_on']} | {same} |")
    lines.append("""
Not taken: the transmittance, depth and transmittance gradient bundles, the ordered tables, the host-pointer forms, per-ray origins, a
profile under rocprofv3 (the key kernel's and the sort's own share), any scene but `-g 64`.
""")
    if resources:
        lines.append("Resources of the key kernel (`tools/kernel_resources.sh raysort`; template argument: INDEXED):\n\n```\n" + resources.rstrip() + "\n```\n")
    return "\n".join(lines)


def windows(fns, calls, repeats, warm=3):
    """ms per call of each fn: `repeats` windows of `calls` back-to-back calls between two stream events, the fns alternating."""
    import torch
    ms = [[] for _ in fns]
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls)
    return [spread(m) for m in ms]


def per_ray(st):
    n = max(st["rays"], 1)
    return {"chunks_tested": round(st["chunks_tested"] / n, 2), "chunks_kept": round(st["chunks_kept"] / n, 2),
            "members_tested": round(st["members_tested"] / n, 1), "list_entries": round(st["lane_entries"] / max(st["short_rays"], 1), 2),
            "pairs": round(st["lane_pairs"] / max(st["short_rays"], 1), 2), "long_rays": st["long_rays"], "scratch_rays": st["scratch_rays"]}


def per_ray_index(ist):
    n = max(ist["groups_tested"] // max(ist["groups"], 1), 1)
    return {"leaves": ist["leaves"], "groups": ist["groups"], "groups_kept": round(ist["groups_kept"] / n, 2),
            "leaves_tested": round(ist["leaves_tested"] / n, 2), "leaves_kept": round(ist["leaves_kept"] / n, 2),
            "members_tested": round(ist["members_tested"] / n, 1)}


def off_and_on(g, nrays, o, origin_per_ray, d, calls, repeats, before=()):
    """One device bundle timed with the index off and on: two contexts on the same scene, windows alternating (behind `before`, other
    paths to alternate with).  o, d: host arrays."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    ctx = [pkg.Renderer(0), pkg.Renderer(0)]
    t_o, t_d = torch.from_numpy(np.ascontiguousarray(o, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(d, f32)).cuda()
    img = [torch.zeros(nrays, dtype=torch.int32, device="cuda") for _ in ctx]
    rad = [torch.zeros((nrays, 4), dtype=torch.float32, device="cuda") for _ in ctx]
    for on, r in enumerate(ctx):
        r.set_gaussians(g)
        r.set_ray_index(on)
    torch.cuda.synchronize()
    run = [lambda k=k: ctx[k].radiance_rays_device(nrays, t_o.data_ptr(), origin_per_ray, t_d.data_ptr(), 0, img[k].data_ptr(), PACK, st) for k in (0, 1)]
    t = windows(list(before) + run, calls, repeats)
    stats = []
    for k, r in enumerate(ctx):
        r.enable_stats(True)
        r.radiance_rays_device(nrays, t_o.data_ptr(), origin_per_ray, t_d.data_ptr(), rad[k].data_ptr(), img[k].data_ptr(), PACK, st)
        stats.append((r.ray_stats(), r.ray_index_stats()))
    torch.cuda.synchronize()
    same = bool(torch.equal(rad[0], rad[1]) and torch.equal(img[0], img[1]))
    lit = int((rad[0][:, :3].sum(1) > 0).sum().item())
    image = img[0].cpu().numpy().view(np.uint32)
    for r in ctx:
        r.close()
    res = {"rays": nrays, "gaussians": len(g), "off_ms": t[-2], "on_ms": t[-1], "off_over_on": round(t[-2]["median"] / t[-1]["median"], 2),
           "identical": same, "lit_rays": lit, "per_ray_off": per_ray(stats[0][0]), "per_ray_on": per_ray(stats[1][0]),
           "per_ray_index": per_ray_index(stats[1][1]), "ray_stats_off": stats[0][0], "ray_stats_on": stats[1][0], "ray_index_stats": stats[1][1]}
    return res, t[:-2], image


def scattered(g, count, seed=5, radius=4.0):
    rng = np.random.default_rng(seed)
    mu = g["mu"][:, :3].astype(np.float64)
    lo, hi = mu.min(0), mu.max(0)
    v = rng.normal(size=(count, 3))
    o = ((lo + hi) / 2 + radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    dd = rng.uniform(lo, hi, size=(count, 3)) - o
    return o, np.ascontiguousarray((dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(f32))


def parts_def(g64, calls, repeats):
    o, d = scattered(g64, 1 << 20)
    res_d, _, _ = off_and_on(g64, len(d), o, 1, d, calls, repeats)
    cam, _ = scene.cli_camera(2048, 2048)
    res_e, _, _ = off_and_on(scene.grid_scene(16), 2048 * 2048, cam.position, 0, directions(cam.plane(), cam.position), calls, repeats)
    cam, _ = scene.cli_camera(256, 256)
    teapot = scene.read_obj(os.path.join(ROOT, "tests", "golden", "test-objects", "teapot.obj"))
    res_f, _, _ = off_and_on(teapot, 256 * 256, cam.position, 0, directions(cam.plane(), cam.position), 2, max(3, repeats // 2))
    return {"scattered": res_d, "g16": res_e, "teapot": res_f}


def parts_bc(g, w, tiles, calls, repeats):
    import torch
    cam, _ = scene.cli_camera(w, w)
    st = torch.cuda.current_stream().cuda_stream
    r = pkg.Renderer(0)
    r.set_gaussians(g)
    r.set_camera_view(w, w, cam.view)
    frame = r.frame_call(2.0 / tiles, 2.0 / tiles, cam.view, cam.position, PACK)
    img_frame = torch.zeros(w * w, dtype=torch.int32, device="cuda")
    origin = cam.position
    d = directions(cam.plane(), origin)
    # (c) two eyes, interleaved: ray 2 p + e is pixel p of the upper half of the frame, seen from eye e
    half = w * (w // 2)
    eyes = np.stack([origin, origin + f32(0.06) * cam.right]).astype(f32)
    plane = [np.asarray(p, f32)[:half] for p in cam.plane()]
    o2 = np.ascontiguousarray(np.tile(eyes, (half, 1)))
    d2 = np.empty((2 * half, 3), f32)
    for e in (0, 1):
        d2[e::2] = directions(plane, eyes[e])
    torch.cuda.synchronize()

    def run_frame():
        frame(img_frame.data_ptr(), st)

    # the bundles get contexts of their own: the paths alternate without disturbing each other's state
    res_b, (t_frame,), img_b = off_and_on(g, w * w, origin, 0, d, calls, repeats, before=[run_frame])
    res_c, _, _ = off_and_on(g, 2 * half, o2, 1, d2, calls, repeats)
    torch.cuda.synchronize()
    # the same frame?  (the camera path culls through three more levels and prunes: both sit inside the documented bounds)
    a = img_frame.cpu().numpy().view(np.uint32)
    ch = lambda x: ((x[:, None] >> np.array([0, 8, 16, 24], np.uint32)) & 255).astype(np.int32)  # noqa: E731
    lsb = int(np.abs(ch(a) - ch(img_b)).max())
    r.close()
    t_b, t_c = res_b["off_ms"], res_c["off_ms"]
    return {"rays": w * w, "frame_device_ms": t_frame, "bundle_one_origin_ms": t_b, "bundle_two_eyes_ms": t_c,
            "bundle_over_frame": round(t_b["median"] / t_frame["median"], 2), "two_eyes_over_frame": round(t_c["median"] / t_frame["median"], 2),
            "indexed_over_frame": round(res_b["on_ms"]["median"] / t_frame["median"], 2),
            "max_u8_difference_to_frame": lsb, "lit_rays": res_b["lit_rays"], "per_ray_one_origin": res_b["per_ray_off"],
            "per_ray_two_eyes": res_c["per_ray_off"], "ray_stats_one_origin": res_b["ray_stats_off"], "ray_stats_two_eyes": res_c["ray_stats_off"],
            "one_origin": res_b, "two_eyes": res_c}


def markdown(res):
    a, bc = res["a"], res["bc"]
    pb, pc = bc["per_ray_one_origin"], bc["per_ray_two_eyes"]
    return f"""# Ray bundles (tools/ray_bundles.py)

(a) {a['rays']} rays at Gaussian centres of `-g 64` (N = {a['gaussians']}), host pointers, call returns after completion:

| call | ms (median, min .. max) |
|---|---|
| `vrt_hip_radiance` (full sum) | {a['full_sum_ms']['median']} ({a['full_sum_ms']['min']} .. {a['full_sum_ms']['max']}, n = {a['full_sum_ms']['n']}) |
| `vrt_hip_radiance_rays` | {a['ray_bundle_ms']['median']} ({a['ray_bundle_ms']['min']} .. {a['ray_bundle_ms']['max']}, n = {a['ray_bundle_ms']['n']}) |

{a['speedup']}x; largest difference of a radiance component {a['max_abs_difference']:.2e} (peak {a['peak_radiance']:.3f}).

(b), (c) {bc['rays']} rays of the `-g 64 -w 2048` frame, device pointers, stream events around back-to-back calls:

| path | ms per call (median, min .. max) | over the camera path |
|---|---|---|
| `vrt_hip_frame_device` (16 x 16 tiles) | {bc['frame_device_ms']['median']} ({bc['frame_device_ms']['min']} .. {bc['frame_device_ms']['max']}) | 1 |
| bundle, one origin | {bc['bundle_one_origin_ms']['median']} ({bc['bundle_one_origin_ms']['min']} .. {bc['bundle_one_origin_ms']['max']}) | {bc['bundle_over_frame']} |
| bundle, two eyes interleaved | {bc['bundle_two_eyes_ms']['median']} ({bc['bundle_two_eyes_ms']['min']} .. {bc['bundle_two_eyes_ms']['max']}) | {bc['two_eyes_over_frame']} |

The bundle's pixels differ from the frame's by at most {bc['max_u8_difference_to_frame']} LSB; {bc['lit_rays']} of its rays are lit.
Per ray, one origin: {pb['chunks_tested']} chunk spheres tested, {pb['chunks_kept']} kept, {pb['members_tested']} Gaussians tested one by one,
{pb['list_entries']} list entries and {pb['pairs']} pairs per lane = ray ray, {pb['long_rays']} rays to the one-wave-per-ray kernel.
Two eyes: {pc['chunks_tested']} / {pc['chunks_kept']} / {pc['members_tested']} / {pc['list_entries']} / {pc['pairs']} / {pc['long_rays']}.

Morton index (`vrt_hip_set_ray_index`) off and on, the same bundle in the same run, windows alternating; ms per call, median (min .. max):

| bundle | rays | N | index off | index on | off / on | same bits | leaves kept per ray (of) | Gaussians tested per ray, off | on | long rays |
|---|---|---|---|---|---|---|---|---|---|---|
| (a) 64 rays, host call | {a['rays']} | {a['gaussians']} | {ms(a['ray_bundle_ms'])} | {ms(a['indexed_ms'])} | {a['off_over_on']} | {a['identical']} | {a['ray_index_stats']['leaves_kept'] / a['rays']:.2f} ({a['ray_index_stats']['leaves']}) | {a['ray_stats']['members_tested'] / a['rays']:.0f} | {a['ray_index_stats']['members_tested'] / a['rays']:.0f} | {a['ray_stats']['long_rays']} |
{index_row('(b) `-g 64` pinhole 2048^2', bc['one_origin'])}
{index_row('(c) `-g 64` two eyes', bc['two_eyes'])}
{index_row('(d) `-g 64` scattered origins', res['def']['scattered'])}
{index_row('(e) `-g 16` pinhole 2048^2', res['def']['g16'])}
{index_row('(f) teapot pinhole 256^2', res['def']['teapot'])}

Indexed (b) over the camera path: {bc['indexed_over_frame']}.
"""


def ms(t):
    return f"{t['median']} ({t['min']} .. {t['max']})"


def index_row(label, r):
    pi = r["per_ray_index"]
    return (f"| {label} | {r['rays']} | {r['gaussians']} | {ms(r['off_ms'])} | {ms(r['on_ms'])} | {r['off_over_on']} | {r['identical']} | "
            f"{pi['leaves_kept']} ({pi['leaves']}) | {r['per_ray_off']['members_tested']} | {pi['members_tested']} | {r['ray_stats_on']['long_rays']} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--transmittance-only", action="store_true")
    ap.add_argument("--depth-only", action="store_true")
    ap.add_argument("--grad-only", action="store_true")
    ap.add_argument("--ordered-only", action="store_true")
    ap.add_argument("--tgrad-only", action="store_true")
    ap.add_argument("--rgrad-only", action="store_true")
    ap.add_argument("--scene-update-only", action="store_true")
    ap.add_argument("--sort-only", action="store_true")
    ap.add_argument("--tangent-only", action="store_true")
    ap.add_argument("--ttangent-only", action="store_true")
    ap.add_argument("--plan-only", action="store_true")
    ap.add_argument("--diag-only", action="store_true")
    ap.add_argument("--diag-cg-only", action="store_true")
    a = ap.parse_args()
    g = scene.grid_scene(a.grid)
    if a.scene_update_only:
        z = part_scene(g)
        print(json.dumps({"scene_update": z}))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "scene_update.json"), "w") as f:
            f.write(json.dumps({"what": "a fitting step with CPU-resident and with cuda-resident parameters, and the device setter alone; see tools/ray_bundles.py (su)",
                                "scene_update": z}) + "\n")
        with open(os.path.join(a.out_dir, "scene_update.md"), "w") as f:
            f.write(markdown_scene(z))
        check_scene(z)
        return
    if a.diag_cg_only:                                              # the CG study of (gn) alone: prints its JSON line, writes nothing
        print(json.dumps({"gn_diag_cg": part_cg()}))
        return
    if a.diag_only:
        z = part_diag(g)
        z["cg"] = part_cg()
        print(json.dumps({"gn_diag": z}))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_gn_diag.json"), "w") as f:
            f.write(json.dumps({"what": "the Gauss-Newton diagonal bundle against the gradient bundle and against four ordered gradient calls with their "
                                        "records squared on the host; see tools/ray_bundles.py (gn)", "gn_diag": z}) + "\n")
        res = os.path.join(a.out_dir, "ray_gn_diag_resources.txt")
        with open(os.path.join(a.out_dir, "ray_gn_diag.md"), "w") as f:
            f.write(markdown_diag(z, open(res).read() if os.path.exists(res) else ""))
        check_diag(z)
        return
    if a.plan_only:
        z = part_plan(g)
        print(json.dumps({"plan": z}))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_plan.json"), "w") as f:
            f.write(json.dumps({"what": "planned against unplanned bundle calls of the same rays; see tools/ray_bundles.py (pl)", "plan": z}) + "\n")
        res = os.path.join(a.out_dir, "ray_plan_resources.md")
        with open(os.path.join(a.out_dir, "ray_plan.md"), "w") as f:
            f.write(markdown_plan(z, open(res).read() if os.path.exists(res) else ""))
        check_plan(z)
        return
    if a.tangent_only:
        z = part_tangent(g)
        print(json.dumps({"tangent": z}))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_tangent.json"), "w") as f:
            f.write(json.dumps({"what": "tangent bundles against radiance and gradient bundles of the same rays; see tools/ray_bundles.py (tn)", "tangent": z}) + "\n")
        res = os.path.join(a.out_dir, "ray_tangent_resources.txt")
        with open(os.path.join(a.out_dir, "ray_tangent.md"), "w") as f:
            f.write(markdown_tangent(z, open(res).read() if os.path.exists(res) else ""))
        check_tangent(z)
        return
    if a.ttangent_only:
        z = part_ttangent(g)
        print(json.dumps({"trans_tangent": z}))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_trans_tangent.json"), "w") as f:
            f.write(json.dumps({"what": "transmittance tangent bundles against transmittance gradient bundles and two transmittance bundles of the same rays; "
                                        "see tools/ray_bundles.py (tt)", "trans_tangent": z}) + "\n")
        res = os.path.join(a.out_dir, "ray_trans_tangent_resources.txt")
        with open(os.path.join(a.out_dir, "ray_trans_tangent.md"), "w") as f:
            f.write(markdown_ttangent(z, open(res).read() if os.path.exists(res) else ""))
        check_ttangent(z)
        return
    if a.sort_only:
        z = part_sort(g, a.width)
        print(json.dumps({"sort": z}))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_sort.json"), "w") as f:
            f.write(json.dumps({"what": "sorted against unsorted bundles of the same rays, Morton index off and on; see tools/ray_bundles.py (so)", "sort": z}) + "\n")
        res = os.path.join(a.out_dir, "ray_sort_resources.txt")
        with open(os.path.join(a.out_dir, "ray_sort.md"), "w") as f:
            f.write(markdown_sort(z, open(res).read() if os.path.exists(res) else ""))
        check_sort(z)
        return
    if a.transmittance_only:
        t = part_t(g)
        print(json.dumps({"t": t}))
        check_t(t)
        return
    if a.grad_only:
        z = part_grad(g)
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_grad.json"), "w") as f:
            f.write(json.dumps({"what": "gradient bundles against radiance bundles of the same rays; see tools/ray_bundles.py (g)", "grad": z}) + "\n")
        res = os.path.join(a.out_dir, "ray_grad_resources.txt")
        with open(os.path.join(a.out_dir, "ray_grad.md"), "w") as f:
            f.write(markdown_grad(z, open(res).read() if os.path.exists(res) else ""))
        print(json.dumps({"grad": z}))
        return
    if a.ordered_only:
        z = part_ordered(g)
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_grad_ordered.json"), "w") as f:
            f.write(json.dumps({"what": "ordered against atomic gradient tables of the same rays; see tools/ray_bundles.py (go)", "ordered": z}) + "\n")
        res = os.path.join(a.out_dir, "ray_grad_ordered_resources.txt")
        with open(os.path.join(a.out_dir, "ray_grad_ordered.md"), "w") as f:
            f.write(markdown_ordered(z, open(res).read() if os.path.exists(res) else ""))
        print(json.dumps({"ordered": z}))
        return
    if a.tgrad_only:
        z = part_tgrad(g)
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_trans_grad.json"), "w") as f:
            f.write(json.dumps({"what": "transmittance gradient bundles against transmittance bundles of the same rays; see tools/ray_bundles.py (tg)", "tgrad": z}) + "\n")
        res = os.path.join(a.out_dir, "ray_trans_grad_resources.txt")
        with open(os.path.join(a.out_dir, "ray_trans_grad.md"), "w") as f:
            f.write(markdown_tgrad(z, open(res).read() if os.path.exists(res) else ""))
        print(json.dumps({"tgrad": z}))
        check_tgrad(z)
        return
    if a.rgrad_only:
        z = part_rgrad(g)
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "ray_grad_rays.json"), "w") as f:
            f.write(json.dumps({"what": "ray gradients against the table call and the forward bundle of the same rays; see tools/ray_bundles.py (rg)", "rgrad": z}) + "\n")

        def side(name, load):
            path = os.path.join(a.out_dir, name)
            return load(open(path).read()) if os.path.exists(path) else None
        with open(os.path.join(a.out_dir, "ray_grad_rays.md"), "w") as f:
            f.write(markdown_rgrad(z, side("ray_grad_rays_existing.json", json.loads), side("ray_grad_rays_pose_fit.json", json.loads),
                                   side("ray_grad_rays_resources.txt", str) or ""))
        print(json.dumps({"rgrad": z}))
        check_rgrad(z)
        return
    if a.depth_only:
        z = part_depth(g)
        print(json.dumps({"depth": z}))
        write_depth(z, a.out_dir)
        check_depth(z)
        return
    res = {"what": "ray bundles against the full sum and against the camera path; see tools/ray_bundles.py",
           "a": part_a(g), "bc": parts_bc(g, a.width, 16, a.calls, a.repeats), "def": parts_def(g, a.calls, a.repeats), "t": part_t(g), "depth": part_depth(g)}
    line = json.dumps(res)
    print(line)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "ray_bundles.json"), "w") as f:
        f.write(line + "\n")
    with open(os.path.join(a.out_dir, "ray_bundles.md"), "w") as f:
        f.write(markdown(res) + markdown_t(res["t"]))
    write_depth(res["depth"], a.out_dir)
    assert res["a"]["speedup"] >= 100.0, "the ray bundle call has to be at least 100 times faster than the full sum on the same rays"
    b = res["bc"]["one_origin"]
    assert b["on_ms"]["median"] < b["off_ms"]["median"], "the indexed call of the -g 64 pinhole bundle has to be faster than the unindexed call"
    check_t(res["t"])
    check_depth(res["depth"])


if __name__ == "__main__":
    main()
