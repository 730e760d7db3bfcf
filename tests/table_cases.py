"""The cases of the table kernel's own limits and their runner (scenes and the float64 model: tests/table_scenes.py; that the cases
sit where they should: tests/test_table_scenes.py; on the GPU: tests/test_gpu_table.py).  Also by hand on an MI355X:

    python tests/table_cases.py 16 [group ...]
    VRT_HIP_TABLE_WAVES=8 python tests/table_cases.py 8 [group ...]          groups: menu stage pairs retry coarsen

The kernel's shape (16 or 8 waves per block) is a function of the frame size, or of VRT_HIP_TABLE_WAVES, which the library reads
once per process: frames of 256 rays take 16 waves, the 8-wave shape needs a process started with the variable set.  One line per
case; the exit code is the number of failed cases (at most 100).

Every case renders 16x16 pixels (four blocks, one tile, cull_eps = 0: every block holds the whole scene) on a context of its own:
  1. the exact kernels of the case's Exp / Erf pair (table step 0): the reference frame;
  2. the table kernel at the case's step with the budget b = max(2.5e-5, bound_ceiling): every block kept on its first attempt,
     `table_nodes` = the model's sum of Gtot (which pins NT, the segment count AND the wave count), `table_skips` inside the model's
     bounds, the frame within b + 5e-6 max(1, peak) of the exact one and within max(TOL, b) max(1, peak) of the oracle on the
     checked pixels;
  or, beyond the menu: every block declined and the frame within 1e-6 of the exact one.
The menu, stage and pair cases run with VRT_HIP_TABLE_ADAPT=1 (no coarsening: the plan is the requested one), the retry and
coarsening cases with the library's default.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.join(HERE, "..", "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

import boundary_scenes as B   # noqa: E402
import table_scenes as T      # noqa: E402
from table_scenes import EXP_FAST, EXP_LIBM, EXP_VCL, ERF_AS, ERF_LIBM, ERF_SPLINE   # noqa: E402

GROUPS = ("menu", "stage", "pairs", "retry", "coarsen")
STAGE_N = {16: (63, 64, 65, 127, 128, 129, 257), 8: (63, 64, 65, 127, 128, 129, 511, 512, 513)}
TABLE_PAIRS = ((EXP_VCL, ERF_AS), (EXP_LIBM, ERF_AS), (EXP_VCL, ERF_LIBM), (EXP_LIBM, ERF_LIBM))
EXACT_PAIRS = ((EXP_VCL, ERF_SPLINE), (EXP_FAST, ERF_AS))     # pairs the table kernel's bound does not cover: they stay exact
PAIR_NAMES = {(EXP_VCL, ERF_AS): "vcl-as", (EXP_LIBM, ERF_AS): "libm-as", (EXP_VCL, ERF_LIBM): "vcl-libm", (EXP_LIBM, ERF_LIBM): "libm-libm",
              (EXP_VCL, ERF_SPLINE): "vcl-spline", (EXP_FAST, ERF_AS): "fast-as"}

_scenes = {}


def scene(oracle, key):
    """('shallow',) | ('deep',) | ('deep', need, which, waves) | ('cloud', cap, n): built once per process."""
    if key not in _scenes:
        if key[0] == "shallow":
            _scenes[key] = T.shallow_stack(oracle)
        elif key[0] == "deep":
            _scenes[key] = T.deep_stack(oracle, *key[1:])
        else:
            _scenes[key] = B.cloud(oracle, key[1], key[2])
    return _scenes[key]


class Case(dict):
    __getattr__ = dict.__getitem__


def _case(oracle, group, name, kind, key, hx, pair=(EXP_VCL, ERF_AS)):
    return Case(group=group, name=name, kind=kind, key=key, hx=float(hx), exp=pair[0], erf=pair[1], sc=scene(oracle, key))


def multi_segment(oracle, dw, nseg):
    """(scene key, step) of the case with `nseg` segments: two intervals past the one-segment limit, the middle of the
    three-segment band, two intervals before the decline limit."""
    sm = T.seg_max(dw)
    need, which = {2: (sm + 3, "min"), 3: (2 * sm + sm // 2, "min"), 8: (8 * sm - 3, "max")}[nseg]
    key = ("deep", need, which, dw)
    return key, T.step_for(scene(oracle, key), need, which)


def menu_cases(oracle, dw):
    out = []
    sh = scene(oracle, ("shallow",))
    for nt, lo, hi in T.bands(dw):
        # the smallest need of the first band is what the largest step the library takes (1) gives
        out.append(_case(oracle, "menu", f"NT{nt}-lo", "table", ("shallow",), 1.0 if nt == 4 else T.step_for(sh, lo + 2, "min")))
        out.append(_case(oracle, "menu", f"NT{nt}-hi", "table", ("shallow",), T.step_for(sh, hi - 2, "max")))
    for nseg in (2, 3, 8):
        key, hx = multi_segment(oracle, dw, nseg)
        out.append(_case(oracle, "menu", f"seg{nseg}", "table", key, hx))
    out.append(_case(oracle, "menu", "beyond", "decline", ("deep",), T.step_for(scene(oracle, ("deep",)), T.need_limit(dw) + 2, "min")))
    return out


def stage_key(dw, n):
    """All-visible cloud of n with its markers on both sides of the multiple of 64 next to n."""
    return ("cloud", 64 * ((n + 1) // 64), n)


def stage_cases(oracle, dw):
    return [_case(oracle, "stage", f"n{n}", "table", stage_key(dw, n), T.STEP_DEFAULT) for n in STAGE_N[dw]]


def pair_cases(oracle, dw):
    out = []
    sh = scene(oracle, ("shallow",))
    _, lo, hi = T.bands(dw)[3]                                                      # NT = 12
    hx1 = T.step_for(sh, (lo + hi) // 2, "min")
    key2, hx2 = multi_segment(oracle, dw, 2)
    for pair in TABLE_PAIRS:
        nm = PAIR_NAMES[pair]
        out.append(_case(oracle, "pairs", f"{nm}-one-segment", "table", ("shallow",), hx1, pair))
        out.append(_case(oracle, "pairs", f"{nm}-two-segments", "table", key2, hx2, pair))
        out.append(_case(oracle, "pairs", f"{nm}-stage", "table", stage_key(dw, T.stage(dw) + 1), T.STEP_DEFAULT, pair))
    for pair in EXACT_PAIRS:
        out.append(_case(oracle, "pairs", f"{PAIR_NAMES[pair]}-stays-exact", "exact-pair", ("shallow",), hx1, pair))
    return out


def cases(oracle, dw, groups=GROUPS):
    out = []
    if "menu" in groups:
        out += menu_cases(oracle, dw)
    if "stage" in groups:
        out += stage_cases(oracle, dw)
    if "pairs" in groups:
        out += pair_cases(oracle, dw)
    if "retry" in groups:
        out.append(_case(oracle, "retry", "ladder", "retry", ("deep",), T.STEP_DEFAULT))
    if "coarsen" in groups:
        out.append(_case(oracle, "coarsen", "defaults", "coarsen", ("deep",), T.STEP_DEFAULT))
    return out


def budget(c, dw):
    return T.budget_of(c.sc, c.hx, dw, c.erf)


def retry_ladder(c, dw):
    """From the ceiling of a context that may coarsen its first attempt, halving, down to 1e-9."""
    b, out = T.bound_ceiling(c.sc, c.hx, dw, c.erf, adapt=T.ADAPT_DEFAULT), []
    while b > 1e-9:
        out.append(b)
        b *= 0.5
    return out + [1e-9]


# ---- the runner ----
def load_pkg():
    """The hyphen-named package directory as module `sgrt_amd` (as tests/conftest.py does; this file runs without pytest too)."""
    if "sgrt_amd" in sys.modules:
        return sys.modules["sgrt_amd"]
    d = os.path.join(HERE, "..", "simd-gaussian-ray-tracing_amd")
    spec = importlib.util.spec_from_file_location("sgrt_amd", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["sgrt_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def _context(pkg, adapt):
    """A fresh context; the library reads VRT_HIP_TABLE_ADAPT when it creates one."""
    old = os.environ.get("VRT_HIP_TABLE_ADAPT")
    if adapt is None:
        os.environ.pop("VRT_HIP_TABLE_ADAPT", None)
    else:
        os.environ["VRT_HIP_TABLE_ADAPT"] = adapt
    try:
        return pkg.Renderer(0)
    finally:
        if old is None:
            os.environ.pop("VRT_HIP_TABLE_ADAPT", None)
        else:
            os.environ["VRT_HIP_TABLE_ADAPT"] = old


def _frame(r, sc, step, b=None):
    r.set_table_step(step)
    if b is not None:
        r.set_table_budget(b)
    _, rad = r.render(sc.origin)
    return rad.reshape(-1, 4).astype(np.float64), r.stats()


def run_case(pkg, oracle, c, dw):
    """(failures, figures) of one case."""
    sc, bad, fig = c.sc, [], {}

    def check(ok, what):
        if not ok:
            bad.append(what)
    r = _context(pkg, None if c.kind in ("retry", "coarsen") else "1")
    try:
        r.set_gaussians(sc.g)
        r.set_plane(sc.w, sc.h, *sc.plane)
        r.tile_gaussians(sc.tw, sc.th, sc.view)
        r.set_options(c.exp, c.erf, 0.0)
        r.set_cull_prune(0.0)
        r.enable_stats(True)
        exact, st0 = _frame(r, sc, 0.0)
        peak = max(1.0, float(exact.max()))
        check(st0["table_blocks"] == 0 and st0["dense_blocks"] == 4, f"exact frame: table_blocks {st0['table_blocks']} dense_blocks {st0['dense_blocks']}")
        if c.kind == "table":
            b = budget(c, dw)
            rad, st = _frame(r, sc, c.hx, b)
            want, (lo, hi) = T.expected_nodes(sc, c.hx, dw), T.skip_bounds(sc, c.hx, dw, c.erf)
            dev = float(np.abs(rad - exact).max())
            _, orad = oracle.render(sc.w, sc.h, sc.plane, sc.origin, sc.g, sc.tiles, exp_kind=c.exp, erf_kind=c.erf, pixels=sc.pixels,
                                    want_image=False, threads=8)
            err = float(np.abs(rad[sc.pixels] - orad).max())
            fig = dict(budget=b, nodes=st["table_nodes"], want=want, skips=st["table_skips"], lo=lo, hi=hi, dev=dev, err=err,
                       blocks=st["table_blocks"], declined=st["table_declined"], retries=st["table_retries"])
            check(st["dense_blocks"] == 4 and st["table_blocks"] + st["table_declined"] == 4, f"dense_blocks {st['dense_blocks']}")
            check(st["table_declined"] == 0 and st["table_retries"] == 0, "a block was declined or retried")
            check(st["table_blocks"] > 0, "no table block")
            check(st["table_nodes"] == want, "table_nodes")
            check(lo <= st["table_skips"] <= hi, "table_skips")
            check(dev <= b + T.NOISE * peak, "table against exact")
            check(err <= max(B.TOL, b) * max(1.0, float(orad.max())), "table against the oracle")
        elif c.kind == "decline":
            rad, st = _frame(r, sc, c.hx, T.BUDGET_DEFAULT)
            dev = float(np.abs(rad - exact).max())
            fig = dict(blocks=st["table_blocks"], declined=st["table_declined"], dev=dev)
            check(st["dense_blocks"] == 4 and st["table_declined"] == 4 and st["table_blocks"] == 0, "not every block declined")
            check(dev <= 1e-6, "declined blocks against exact")
        elif c.kind == "exact-pair":
            rad, st = _frame(r, sc, c.hx, T.BUDGET_DEFAULT)
            fig = dict(blocks=st["table_blocks"], dense=st["dense_blocks"], declined=st["table_declined"])
            check(st["dense_blocks"] == 4 and st["table_blocks"] == 0 and st["table_declined"] == 0, "the pair went through the table kernel")
        elif c.kind == "retry":
            ladder, rungs = retry_ladder(c, dw), []
            for b in ladder:
                rad, st = _frame(r, sc, c.hx, b)
                dev = float(np.abs(rad - exact).max())
                rungs.append((st["table_retries"], st["table_declined"]))
                check(st["dense_blocks"] == 4 and st["table_blocks"] + st["table_declined"] == 4, f"budget {b:.3g}: blocks")
                check(dev <= b + T.NOISE * peak, f"budget {b:.3g}: deviation {dev:.3g}")
            fig = dict(top=ladder[0], rungs="".join(f"{a}{d}" for a, d in rungs))     # per rung: retries, declined
            check(any(a > 0 and d < 4 for a, d in rungs), "no rung with a successful second attempt")
            check(rungs[0][0] == 0 and rungs[0][1] == 0, "the top rung retried")
            check(rungs[-1][1] == 4, "the bottom rung kept a block")
        else:   # coarsen: the library's defaults; whether the estimate lets a block coarsen cannot be derived without the kernel
            rad, st = _frame(r, sc, c.hx, T.BUDGET_DEFAULT)
            dev = float(np.abs(rad - exact).max())
            fig = dict(coarser=st["table_coarser"], blocks=st["table_blocks"], declined=st["table_declined"], retries=st["table_retries"],
                       nodes=st["table_nodes"], dev=dev)
            check(st["dense_blocks"] == 4 and st["table_blocks"] + st["table_declined"] == 4, "blocks")
            check(dev <= T.BUDGET_DEFAULT + T.NOISE * peak, "deviation")
    finally:
        r.close()
    return bad, fig


def run(pkg, oracle, dw, groups=GROUPS, out=print):
    """Render the cases of `groups` for the shape of `dw` waves; the names of the failed ones."""
    forced = os.environ.get("VRT_HIP_TABLE_WAVES")
    if (forced or "16") != str(dw):
        raise RuntimeError(f"this process renders with VRT_HIP_TABLE_WAVES={forced}: start one for {dw} waves")
    failed = []
    for c in cases(oracle, dw, groups):
        bad, fig = run_case(pkg, oracle, c, dw)
        figures = " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in fig.items())
        out(f"waves={dw} {c.group}/{c.name} n={c.sc.n} {PAIR_NAMES[(c.exp, c.erf)]} step={c.hx:.5g}: {figures} {'FAIL: ' + '; '.join(bad) if bad else 'ok'}")
        if bad:
            failed.append(f"{c.group}/{c.name}")
    return failed


if __name__ == "__main__":
    import time
    import oracle as O
    O.build()
    t0 = time.perf_counter()
    failed = run(load_pkg(), O, int(sys.argv[1]), tuple(sys.argv[2:]) or GROUPS, out=lambda s: print(s, flush=True))
    print(f"{len(failed)} failed {failed} in {time.perf_counter() - t0:.1f} s", flush=True)
    sys.exit(min(len(failed), 100))
