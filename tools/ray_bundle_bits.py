#!/usr/bin/env python3
"""The raw float32 bits of all three kinds of ray bundle, for comparing two builds of the library.  Needs the GPU.

    VRT_HIP_LIB=<build A>/libvrt_hip.so python tools/ray_bundle_bits.py --out a.npz
    VRT_HIP_LIB=<build B>/libvrt_hip.so python tools/ray_bundle_bits.py --out b.npz
    cmp a.npz b.npz            (python tools/ray_bundle_bits.py --out b.npz --against a.npz names the results that differ)

Radiance, transmittance and depth bundles of 130 rays (three waves, the last with two rays) through the scenes of
tests/ray_bundle_scenes.py that sit on the kernels' capacities: stack_with_side at RAY_PL and RAY_PL + 1 (lane = ray lists full and
one over), wide_stack at RAY_LCAP and RAY_LCAP + 1 (one wave per ray: the list in LDS, and one entry in the scratch slot), and
scattered rays through `-g 16` (lists from a handful to far beyond RAY_PL in one wave).  Every bundle with one origin and with an origin
per ray, the Morton index off and on, under every Exp / Erf pair the kernels are instantiated for; the tables of the transmittance and
depth bundles shared and per ray, with 1, 4 and 7 values per ray (either side of the 4 that ride on one walk of a list).  The file
holds the same bytes whenever the results do: the members are stored in name order with a fixed date.

--grad adds (--grad-only: records alone) the two kinds of gradient bundle, under the four Exp / Erf pairs they have kernels for.  Their
tables are sums of float atomics, so only bundles whose sums CAN come out the same twice are run: one ray (small 9 of
tests/grad_bundle_scenes.py; the axial ray of the stack at RAY_PL and RAY_PL + 1 and of the wide stack at RAY_LCAP + 1, the one-wave-
per-ray kernels' case with one entry in the scratch slot), and one wave of 64 near-axial rays that all keep the stack of RAY_PL (one row
per list position in every lane: the wave-summed deposit).  The transmittance kind with 1, 4 and 5 samples -- the wide stack's ray
also with NSC and NSC + 1, one and two chunks of the one-wave-per-ray kernel: two adds per address from one lane -- in both `wrt`
modes, with and without the table and the per-sample output, which is stored, not added.  Every one of these calls again with the
ray rows (want_rays: the RAYS kernels), rows alone and rows with the table -- rows alone for the wave of 64; the rows are stored, not
added, and compare on every bundle.  Then the ORDERED kernels (set_grad_ordered: reproducible by contract): the same bundles and three
of the 130-ray bundles above (the stack at RAY_PL + 1, the wide stack at RAY_LCAP + 1 and the scattered rays: long and short rays in
one wave, whole waves and a ragged last one, the scratch slot), both kinds of gradient without and with the ray rows, the wide stacks
also with NSC + 1 samples -- the table, the ray rows, and the count and sha256 of grad_records() (130 rays x 1025 kept x 2 records are
12 MB a call).  What is reproducible without the contract is for two runs of ONE build to say:

    VRT_HIP_LIB=<build A> ... --grad-only --out a1.npz
    VRT_HIP_LIB=<build A> ... --grad-only --out a2.npz --against a1.npz
    VRT_HIP_LIB=<build B> ... --grad-only --out b.npz --against a1.npz --among a2.npz     (compares what a1 and a2 agree on)"""
import argparse
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import __graft_entry__ as ge  # noqa: E402
import oracle  # noqa: E402  (its scene constructor alone: nothing of it is compiled or loaded)
import grad_bundle_scenes as G  # noqa: E402
import ray_bundle_scenes as S  # noqa: E402

pkg = ge._load_pkg()
from sgrt_amd import scene  # noqa: E402

NRAYS = 130
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (3, 1), (1, 2), (1, 3), (1, 4)]   # VRT_DISPATCH_EXP_ERF (csrc/vrt_kernels_common.hpp)
COUNTS = (1, 4, 7)
GRAD_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]   # VRT_DISPATCH_GRAD_PAIR
GRAD_COUNTS = (1, 4, 5)                         # either side of the 4 samples that ride on one walk of a list
NSC = 512                                       # csrc/vrt_ray_trans_grad_kernel.hip: samples per chunk of the one-wave-per-ray kernel
CHUNK_COUNTS = (NSC, NSC + 1)                   # one chunk exactly, and a second chunk of one sample: the wide stack's ray alone
f32 = np.float32


def near_axis_rays():
    """wide_rays() and more of their kind: every one keeps the whole wide stack."""
    rng = np.random.default_rng(77)
    target = np.concatenate([[[0.0, 0.0, 1.0], [0.05, 0.02, 1.0], [-0.03, 0.06, 1.0]],
                             np.column_stack([rng.normal(size=(NRAYS - 3, 2)) * 0.04, np.ones(NRAYS - 3)])])
    return S.STACK_ORIGIN, S.normalise(target - S.STACK_ORIGIN.astype(np.float64))


def cases():
    """(name, scene, origin [3], origins [NRAYS, 3], dirs [NRAYS, 3])"""
    grid = scene.grid_scene(16)
    so, sd = S.scattered_rays(grid, count=NRAYS)
    out = [("stack%d" % k, S.stack_with_side(oracle, k), *S.stack_rays(nmiss=NRAYS - 2)) for k in (S.RAY_PL, S.RAY_PL + 1)]
    out += [("wide%d" % n, S.wide_stack(oracle, S.RAY_LCAP, n).g, *near_axis_rays()) for n in (S.RAY_LCAP, S.RAY_LCAP + 1)]
    out = [(name, g, o, np.ascontiguousarray(np.tile(o, (NRAYS, 1))), d) for name, g, o, d in out]
    return out + [("scattered", grid, so[0].copy(), so, sd)]


def tables(n):
    """{'shared' / 'per_ray': (sample distances, transmittance levels)} with n values per ray"""
    s = np.linspace(0.5, 6.0, n).astype(f32)
    tau = np.linspace(0.97, 0.35, n).astype(f32)
    k = (1.0 + 0.003 * np.arange(NRAYS))[:, None]
    return {"shared": (s, tau), "per_ray": ((s[None, :] * k).astype(f32), np.clip(tau[None, :] / k, 0.0, 1.0).astype(f32))}


def run():
    res = {}
    r = pkg.Renderer(0)
    for name, g, o1, on, d in cases():
        assert len(d) == NRAYS and on.shape == (NRAYS, 3)
        r.set_gaussians(g)
        r.set_options(1, 1, S.CULL_EPS)
        r.set_ray_index(0)
        r.enable_stats(True)
        r.radiance_rays(on, d)
        st = r.ray_stats()
        r.enable_stats(False)
        print(f"{name}: {len(g)} Gaussians, {st['short_rays']} rays lane = ray, {st['long_rays']} one wave per ray, {st['scratch_rays']} of them past RAY_LCAP")
        for exp_kind, erf_kind in PAIRS:
            r.set_options(exp_kind, erf_kind, S.CULL_EPS)
            for index in (0, 1):
                r.set_ray_index(index)
                for form, o in (("one_origin", o1), ("origin_per_ray", on)):
                    key = f"{name}/exp{exp_kind}_erf{erf_kind}/index{index}/{form}"
                    res[key + "/radiance"] = r.radiance_rays(o, d)
                    for n in COUNTS:
                        for which, (s, tau) in tables(n).items():
                            res[f"{key}/transmittance/{n}_{which}"] = r.transmittance_bundle(o, d, s)
                            res[f"{key}/depth/{n}_{which}"] = r.depth_bundle(o, d, tau)
    r.close()
    return {k: np.ascontiguousarray(v, f32).view(np.uint32) for k, v in res.items()}


def grad_cases():
    """(name, scene, origin [3], dirs [rays, 3], sample counts): bundles whose table sums can be reproducible"""
    small = G.small(oracle, 9)
    o, d = S.stack_rays(nmiss=0)
    out = [("small9", small.g, small.o, small.d[:1], GRAD_COUNTS)]
    out += [("stack%d" % k, S.stack_with_side(oracle, k), o, d[:1], GRAD_COUNTS) for k in (S.RAY_PL, S.RAY_PL + 1)]
    out.append(("wide%d" % (S.RAY_LCAP + 1), S.wide_stack(oracle, S.RAY_LCAP, S.RAY_LCAP + 1).g, *(a[:1] if a.ndim == 2 else a for a in S.wide_rays()),
                GRAD_COUNTS + CHUNK_COUNTS))
    ang = np.arange(64) * (2 * np.pi / 64)
    target = np.stack([0.02 * np.cos(ang) * (np.arange(64) % 4) / 3, 0.02 * np.sin(ang) * (np.arange(64) % 4) / 3, np.ones(64)], 1)
    out.append(("stack%d_wave" % S.RAY_PL, S.stack_with_side(oracle, S.RAY_PL), o, S.normalise(target - o.astype(np.float64)), GRAD_COUNTS))
    return out


def table_of(cols):
    """grad_columns undone: the table [N, GRAD_STRIDE]"""
    return np.column_stack([cols["albedo"], cols["mu"], cols["sigma"], cols["magnitude"]])


def rows_of(rows):
    """ray_grad_columns undone: [nrays, 6]"""
    return np.column_stack([rows["origin"], rows["dir"]])


def records_of(r):
    """the count and the sha256 of grad_records() of the last ordered call, as 9 words"""
    gauss, ray, rows = r.grad_records()
    digest = hashlib.sha256(gauss.tobytes() + ray.tobytes() + rows.tobytes()).digest()
    return np.concatenate([[len(gauss)], np.frombuffer(digest, np.uint32)]).astype(np.uint32).view(f32)


def run_grad_ordered(r, res):
    """The ORDERED kernels, without and with the ray rows; the switch is off again behind them."""
    bundles = [(name, g, o, d, GRAD_COUNTS + ((NSC + 1,) if name.startswith("wide") else ())) for name, g, o, d, _ in grad_cases()]
    bundles += [(f"{name}_{NRAYS}rays", g, on, d, GRAD_COUNTS + ((NSC + 1,) if name.startswith("wide") else ()))
                for name, g, _, on, d in cases() if name in ("stack%d" % (S.RAY_PL + 1), "wide%d" % (S.RAY_LCAP + 1), "scattered")]
    r.set_grad_ordered(True)
    for name, g, o, d, counts in bundles:
        nrays = len(d)
        r.set_gaussians(g)
        rng = np.random.default_rng(7000 + len(g) + nrays)
        gr = rng.uniform(-1.0, 1.0, size=(nrays, 4)).astype(f32)
        gTs = {ns: rng.uniform(-1.0, 1.0, size=(nrays, ns)).astype(f32) for ns in counts}
        for exp_kind, erf_kind in GRAD_PAIRS:
            r.set_options(exp_kind, erf_kind, S.CULL_EPS)
            for index in (0, 1):
                r.set_ray_index(index)
                key = f"gradord/{name}/exp{exp_kind}_erf{erf_kind}/index{index}"
                res[key + "/radiance/table"] = table_of(r.radiance_rays_grad(o, d, gr))
                res[key + "/radiance/records"] = records_of(r)
                cols, rows = r.radiance_rays_grad(o, d, gr, True, True)
                res[key + "/radiance/rays/table"], res[key + "/radiance/rays/rows"], res[key + "/radiance/rays/records"] = table_of(cols), rows_of(rows), records_of(r)
                for ns in counts:
                    s = np.tile(np.linspace(0.5, 6.0, ns).astype(f32), (nrays, 1))
                    depth = r.depth_bundle(o, d, np.linspace(0.97, 0.35, ns).astype(f32))
                    for mode, wrt, at in (("T", pkg.TGRAD_T, s), ("depth", pkg.TGRAD_DEPTH, depth)):
                        at_key = f"{key}/{mode}/ns{ns}"
                        res[at_key + "/table"] = table_of(r.transmittance_bundle_grad(o, d, at, gTs[ns], wrt, True, True, True)[0])
                        res[at_key + "/records"] = records_of(r)
                        cols, _, rows = r.transmittance_bundle_grad(o, d, at, gTs[ns], wrt, True, True, False, True)
                        res[at_key + "/rays/table"], res[at_key + "/rays/rows"], res[at_key + "/rays/records"] = table_of(cols), rows_of(rows), records_of(r)
        st = r.grad_ordered_stats()
        print(f"ordered {name}: {nrays} rays, the last call: " + ", ".join(f"{k} {v}" for k, v in st.items()))
    r.set_grad_ordered(False)


def run_grad():
    res = {}
    r = pkg.Renderer(0)
    for name, g, o, d, counts in grad_cases():
        nrays = len(d)
        r.set_gaussians(g)
        r.set_options(1, 1, S.CULL_EPS)
        r.set_ray_index(0)
        r.enable_stats(True)
        r.radiance_rays(o, d)
        st = r.ray_stats()
        r.enable_stats(False)
        print(f"grad {name}: {len(g)} Gaussians, {nrays} rays: {st['short_rays']} lane = ray ({st['lane_entries']} list entries), {st['long_rays']} one wave per ray, "
              f"{st['scratch_rays']} of them past RAY_LCAP")
        rng = np.random.default_rng(900 + len(g) + nrays)
        gr = rng.uniform(-1.0, 1.0, size=(nrays, 4)).astype(f32)
        for exp_kind, erf_kind in GRAD_PAIRS:
            r.set_options(exp_kind, erf_kind, S.CULL_EPS)
            for index in (0, 1):
                r.set_ray_index(index)
                key = f"grad/{name}/exp{exp_kind}_erf{erf_kind}/index{index}"
                res[key + "/radiance/table"] = table_of(r.radiance_rays_grad(o, d, gr))
                res[key + "/radiance/rays_alone/rows"] = rows_of(r.radiance_rays_grad(o, d, gr, False, True)[1])
                if nrays == 1:
                    cols, rows = r.radiance_rays_grad(o, d, gr, True, True)
                    res[key + "/radiance/rays_table/table"], res[key + "/radiance/rays_table/rows"] = table_of(cols), rows_of(rows)
                for ns in counts:
                    s = np.tile(np.linspace(0.5, 6.0, ns).astype(f32), (nrays, 1))
                    depth = r.depth_bundle(o, d, np.linspace(0.97, 0.35, ns).astype(f32))    # +inf where a level is never reached: contributes nothing
                    gT = rng.uniform(-1.0, 1.0, size=(nrays, ns)).astype(f32)
                    gT[0, ns - 1] = 0.0 if ns > 1 else gT[0, 0]                              # a sample that is skipped exactly
                    for mode, wrt, at in (("T", pkg.TGRAD_T, s), ("depth", pkg.TGRAD_DEPTH, depth)):
                        for what, table, per_sample in (("both", True, True), ("table", True, False), ("grad_s", False, True)):
                            cols, gs = r.transmittance_bundle_grad(o, d, at, gT, wrt, True, table, per_sample)
                            if table:
                                res[f"{key}/{mode}/ns{ns}/{what}/table"] = table_of(cols)
                            if per_sample:
                                res[f"{key}/{mode}/ns{ns}/{what}/grad_s"] = gs
                        res[f"{key}/{mode}/ns{ns}/rays_alone/rows"] = rows_of(r.transmittance_bundle_grad(o, d, at, gT, wrt, True, False, False, True)[2])
                        if nrays == 1:
                            cols, gs, rows = r.transmittance_bundle_grad(o, d, at, gT, wrt, True, True, True, True)
                            res[f"{key}/{mode}/ns{ns}/rays_table/table"], res[f"{key}/{mode}/ns{ns}/rays_table/rows"] = table_of(cols), rows_of(rows)
                            res[f"{key}/{mode}/ns{ns}/rays_table/grad_s"] = gs
    run_grad_ordered(r, res)
    r.close()
    return {k: np.ascontiguousarray(v, f32).view(np.uint32) for k, v in res.items()}


def write(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[name], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--against", help="an earlier --out file: name the results whose bits differ, exit 1 if any does")
    ap.add_argument("--among", help="with --against: another --out file of the build that wrote --against; only the results on which the two agree are compared")
    ap.add_argument("--grad", action="store_true", help="the gradient bundles as well")
    ap.add_argument("--grad-only", action="store_true", help="the gradient bundles alone")
    a = ap.parse_args()
    arrays = {} if a.grad_only else run()
    if a.grad or a.grad_only:
        arrays.update(run_grad())
    write(a.out, arrays)
    finite = sum(int(np.isfinite(v.view(f32)).sum()) for v in arrays.values())
    print(f"{len(arrays)} results, {sum(v.size for v in arrays.values())} values ({finite} finite) from {pkg.LIB_PATH} -> {a.out}")
    if a.against:
        other = np.load(a.against)
        names = sorted(set(arrays) | set(other.files))
        if a.among:
            twin = np.load(a.among)
            names = [k for k in names if k in other.files and k in twin.files and np.array_equal(other[k], twin[k])]
            digest = hashlib.sha256()
            for k in names:
                digest.update(k.encode() + other[k].tobytes())
            print(f"{len(names)} of {len(other.files)} results are the same in {a.against} and {a.among}: sha256 of their names and bits {digest.hexdigest()}")
        bad = [k for k in names if k not in arrays or k not in other.files or not np.array_equal(arrays[k], other[k])]
        for k in bad:
            print("differs", k)
        print(f"{len(bad)} of {len(names)} results differ from {a.against}")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
