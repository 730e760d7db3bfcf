"""Generates tests/golden/approx_ref.npz and tests/golden/approx_edges.npz from the REAL reference approximations
(/root/reference/src/vrt/approx.{h,cpp} compiled in place into oracle/_ref by oracle/Makefile).

Run in the build container (where /root/reference exists):  python tests/golden/gen_approx_golden.py
Grids: the reference's own accuracy experiment (tests/accuracy.cpp:19, 35-39: erf on [-6,6] step .1,
exp on [-16,0] step .1) plus a denser/wider sweep.  Only numbers are stored -- no reference source.
approx_edges.npz: the same functions at the edges of their definitions (`edge_inputs`) -- finite inputs only: the reference is a
-ffast-math build and defines nothing at inf and NaN.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import oracle as O  # noqa: E402

O.build()
assert O.ref_lib() is not None, "oracle/_ref missing: needs /root/reference"

erf_x = np.unique(np.concatenate([np.arange(-6, 6.0001, 0.1), np.linspace(-9, 9, 1153), [0.0, -0.0, 1e-8, -1e-8]])).astype(np.float32)
exp_x = np.unique(np.concatenate([np.arange(-16, 0.0001, 0.1), np.linspace(-87, 0.5, 1401)])).astype(np.float32)
out = dict(erf_x=erf_x, exp_x=exp_x)
for key, fn in [("as_erf", "ref_as_erf"), ("simd_as_erf", "ref_simd_as_erf"), ("spline_erf", "ref_spline_erf"),
                ("spline_erf_mirror", "ref_spline_erf_mirror"), ("taylor_erf", "ref_taylor_erf"),
                ("simd_spline_erf", "ref_simd_spline_erf"), ("simd_spline_erf_mirror", "ref_simd_spline_erf_mirror"),
                ("simd_taylor_erf", "ref_simd_taylor_erf")]:
    out[key] = O.ref_map(fn, erf_x)
for key, fn in [("vcl_exp", "ref_simd_vcl_exp"), ("fast_exp", "ref_fast_exp"), ("spline_exp", "ref_spline_exp"),
                ("simd_fast_exp", "ref_simd_fast_exp"), ("simd_spline_exp", "ref_simd_spline_exp")]:
    out[key] = O.ref_map(fn, exp_x)
# libm columns (the template defaults expf/erff of rt.h:32), float64 math rounded to float
import math
out["libm_erf"] = np.array([math.erf(float(v)) for v in erf_x], np.float32)
out["libm_exp"] = np.exp(exp_x.astype(np.float64)).astype(np.float32)
np.savez_compressed(os.path.join(HERE, "approx_ref.npz"), **out)
print("wrote approx_ref.npz:", {k: v.shape for k, v in out.items()})


# ---- approx_edges.npz -------------------------------------------------------------------------------------------------------
def around(v):
    """v as float32, and its float32 neighbours either side"""
    v = np.asarray(v, np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])


def edge_inputs():
    """(erf_x, exp_x): +-0, the smallest normal and a subnormal, +-1e-8, every piece border of the splines (erf: -2.9 : 0.6 : 3.1; exp: -9 : 1 : -5,
    -5 : 0.5 : -2, -2 : 0.25 : 0) and |x| = 2 of the Taylor erf with their float32 neighbours, +-4.5, +-6, +-10, and for the exps +-87.3 (vcl_exp's
    limit), +-88.7 and the two clamps of fast_exp -- a x + b = 2^23 at x = -126.956 ln 2, = 255 * 2^23 at x = 128.044 ln 2 -- with neighbours"""
    # (the subnormals 2^-140 by their bits: with the reference library loaded, this process converts them to 0)
    tiny = np.concatenate([np.array([0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 1e-8, -1e-8], np.float32), np.array([1 << 9, 1 << 31 | 1 << 9], np.uint32).view(np.float32)])
    far = np.array([4.5, -4.5, 6, -6, 10, -10], np.float32)
    erf_borders = np.array([-2.9, -2.3, -1.7, -1.1, -0.5, 0.1, 0.7, 1.3, 1.9, 2.5, 3.1, -2.0, 2.0], np.float32)
    exp_borders = np.concatenate([np.arange(-9, -5, 1.0), np.arange(-5, -2, 0.5), np.arange(-2, 0.01, 0.25)]).astype(np.float32)
    ln2 = np.log(2.0)
    clamps = np.array([(1 - (127 - 0.043677448)) * ln2, (255 - (127 - 0.043677448)) * ln2], np.float32)
    limits = np.array([87.3, -87.3, 88.7, -88.7], np.float32)
    erf_x = np.concatenate([tiny, far, around(erf_borders)])
    exp_x = np.concatenate([tiny, far, around(exp_borders), around(limits), around(clamps), clamps - np.float32(0.01), clamps + np.float32(0.01)])
    return erf_x.astype(np.float32), exp_x.astype(np.float32)


erf_x, exp_x = edge_inputs()
assert np.isfinite(erf_x).all() and np.isfinite(exp_x).all() and (erf_x.view(np.uint32) & 0x7FFFFFFF == 1 << 9).sum() == 2
edges = dict(erf_x=erf_x, exp_x=exp_x)
for key, fn in [("as_erf", "ref_as_erf"), ("spline_erf", "ref_spline_erf"), ("spline_erf_mirror", "ref_spline_erf_mirror"), ("taylor_erf", "ref_taylor_erf")]:
    edges[key] = O.ref_map(fn, erf_x)
for key, fn in [("vcl_exp", "ref_simd_vcl_exp"), ("fast_exp", "ref_fast_exp"), ("spline_exp", "ref_spline_exp")]:
    edges[key] = O.ref_map(fn, exp_x)
edges["libm_erf"] = np.array([math.erf(float(v)) for v in erf_x], np.float32)
with np.errstate(over="ignore"):
    edges["libm_exp"] = np.exp(exp_x.astype(np.float64)).astype(np.float32)
np.savez_compressed(os.path.join(HERE, "approx_edges.npz"), **edges)
print("wrote approx_edges.npz:", {k: v.shape for k, v in edges.items()})
