"""State-machine fuzz of the ray-bundle family: ONE long-lived context against fresh ones.

    python tests/bundle_state_scenes.py [seed] [steps]

runs it by hand on an MI355X and prints one line per step; tests/test_gpu_bundle_state.py runs the committed seeds,
tests/test_bundle_state_scenes.py checks on the CPU, with a stub in place of the library, that the sequences reach what they claim and
that `run` reports the ways such state can leak.

The long-lived context A receives a seeded sequence of state changes -- scene (host setter, vrt_hip_set_gaussians_device on the current
or on a side stream), bundle, Exp / Erf pair and cull_eps, the switches set_ray_index / set_ray_sort / set_grad_ordered / enable_stats,
ray plans made, bound (strict or with keep_lists), unbound and destroyed, a small frame in between -- and after each one runs ONE bundle
entry point: host form, device form, several device calls back to back without a wait, or ("nosync") enqueued on a side stream and NOT
waited for, so that the next step's state change is applied while it is in flight; it is judged after that.  Three streams take turns.
Between a nosync bundle and what follows it the harness waits for nothing: the expectations of ALL steps are computed before A takes its
first step (a fresh context waits for the whole device when it is made, used and closed), the device setter's arrays of every scene are
staged once, staging a call's inputs waits for torch's current stream alone, and the next step's device form is enqueued BEFORE the
bundle in flight is waited for -- so only quiesce / wait_for_last_stream in the library keep a bundle in flight from seeing the next
scene, and a bundle on another stream from sharing its queue, counters and scratch.
The expectation comes from a fresh context B configured PLAIN: host setter, index off, sort off, no plan, ordered on (for the tables).
include/vrt_hip.h promises the same bits under every one of those switches.  The one exception is a bound plan that is no longer the
cull of the current (scene, options, rays) and is still admitted -- a keep_lists plan behind a scene or option change, or other rays of
the plan's count: there the value is the sum over the plan's lists, and B replays how A got there (old state, make the plan, new state).

Per step: bit for bit everything the header calls reproducible (radiance, pixels, T, depth, ray rows, grad_s, tangents, ordered
tables with their records and mismatches == 0, ray_order of a sorted bundle, a new plan's lists); the SAME_STATS fields of ray_stats
when stats are on; a float-atomic table (ordered off) against B's ordered one within the bound the suites grant two runs of one atomic
call, 2 * grad_bundle_scenes.bound(S) or 2 * trans_grad_bundle_scenes.bound(S) of the float64 model (`Reference`); a refused step must
be refused by both with the same code, leave every output word as it was, and A must pass the next step.  On steps whose scene has at
most 300 Gaussians and whose bundle has at most 130 rays B itself is held to the oracle's full sum (ray_bundle_scenes.tolerance,
transmittance_bundle_scenes.tolerance), so that A == B is never two wrong answers agreeing.

What is NOT compared, and why: the VALUES of a float-atomic table where the float64 model does not qualify (more than 300 Gaussians or
130 rays, cull_eps = 1e-6, a pair the gradient suites state no bound for, lists replayed from a plan: the model costs minutes there, and
no other bound exists) and of gn_diag's (only its own suite states a bound for it) -- such a table is still held to the ordered one's
shape, to the same entries finite and to exact zeros in the rows no ray keeps, and its ray rows and grad_s bit for bit; the float64 check under
cull_eps = 1e-6 (the cull may then drop 3 * cull_eps * N, which the parity tolerance does not cover); statistics, records and the order
of a nosync step (they are read after the next state change, which the header does not cover).

This module imports no GPU code at module level: `Gpu` imports torch when it is made.
"""
import collections
import dataclasses
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ray_bundle_scenes as R           # noqa: E402
import ray_sort_scenes as RS            # noqa: E402
from ray_bundle_scenes import RAY_PL, RAY_LCAP  # noqa: E402

# ---- the families: scenes and bundles whose bounds the suites state ----
CLOUDS = (0, 1, 64, 65, 300, 4097)      # 4097: 65 chunks or leaves -- the second 64-wide pass of ray_long_cull, two index groups
TWINS = (65, 300)                       # "cloud-N~": the same cloud a small step further, as a fit moves it: another scene of the SAME N
STACK, WIDE = f"stack-{RAY_PL + 1}", f"wide-{RAY_LCAP + 1}"
SCENES = tuple(f"cloud-{n}" for n in CLOUDS) + tuple(f"cloud-{n}~" for n in TWINS) + (STACK, WIDE)
N_OF = {**{f"cloud-{n}": n for n in CLOUDS}, **{f"cloud-{n}~": n for n in TWINS}, STACK: RAY_PL + 1 + 5, WIDE: RAY_LCAP + 1}
SCENE_WEIGHT = {"cloud-4097": 3.0, STACK: 2.0, WIDE: 2.0}      # the sizes at which the kernels change: drawn more often
COUNTS = (1, 64, 65, 130, 1024)
EPS = (1e-9, 1e-9, 0.0, 1e-6)
PAIRS = [(1, 1)] * 4 + [(0, 0), (2, 1), (1, 4)]      # (Exp, Erf) as the package numbers them: vcl / A&S, libm / libm, and two with jumps
SMOOTH = ((1, 1), (0, 0), (1, 0), (0, 1))            # {vcl_exp, expf} x {A&S erf, erff}: the pairs a derivative is taken under
MODELLED = {(1, 1): "vcl-as", (0, 0): "libm-libm"}   # the pairs the gradient suites' float64 models and bounds are stated for
SAMPLES = np.array([3.5, 4.4, 5.0, 5.6, 6.5], np.float32)      # tests/test_gpu_ray_sort.py's: through the scenes from z = -4
LEVELS = np.array([0.9, 0.5, 0.1], np.float32)
SAME_STATS = ("rays", "short_rays", "long_rays", "lane_entries", "lane_pairs", "scratch_rays")

OPS = ("scene", "bundle", "options", "index", "sort", "ordered", "stats", "plan", "plan-keep", "unplan", "frame", "none")
OP_P = (.17, .13, .10, .07, .07, .07, .05, .07, .08, .05, .06, .08)
CALLS = ("radiance", "T shared", "T per ray", "depth", "grad", "tgrad", "tangent", "ttangent T", "ttangent depth", "gn_diag")
DERIVATIVES = ("grad", "tgrad", "tangent", "ttangent T", "ttangent depth", "gn_diag")
TABLES = ("grad", "tgrad", "gn_diag")
HOWS = ("host", "device", "repeat", "nosync")
HOW_P = (.3, .25, .2, .25)
NSTREAMS = 3
INVALID = -1                             # VRT_HIP_ERR_INVALID
# The committed (seed, steps): tests/test_bundle_state_scenes.py holds their union to the coverage the GPU suite claims, and
# tests/test_gpu_bundle_state.py runs one case each.  A case that takes more than a few seconds on the GPU gets fewer steps and another seed
# the rest -- never larger shapes.
CASES = ((6, 40), (9, 40), (12, 40), (20, 40), (22, 40), (26, 40), (33, 40), (34, 40))

Bundle = collections.namedtuple("Bundle", "aim count per_ray seed")      # rays aimed at the Gaussians of scene `aim`
Plan = collections.namedtuple("Plan", "keep scene opt bundle gen")       # ... and what it was made under


@dataclasses.dataclass
class State:
    scene: str = "cloud-65"
    setter: str = "host"                 # host | device (vrt_hip_set_gaussians_device on the current stream) | side (on a side stream)
    opt: tuple = (1, 1, 1e-9)            # Exp, Erf, cull_eps
    index: bool = False
    sort: bool = False
    ordered: bool = False
    stats: bool = False
    plan: Plan = None
    bundle: Bundle = Bundle("cloud-65", 65, False, 0)
    gen: int = 0                         # scene sets and option changes so far: what makes a strict plan stale


def replayed(st):
    """The bound plan is not the cull of the current (scene, options, rays): a planned call sums over OTHER lists than a plain one"""
    p = st.plan
    return p is not None and (p.scene, p.opt, p.bundle) != (st.scene, st.opt, st.bundle)


def verdict(st, call):
    """None, or why the library must refuse `call` in state st -- decided from the state alone, in the library's order of checks"""
    p = st.plan
    if p is not None:
        if p.bundle.count != st.bundle.count:
            return "count"
        if p.keep:
            if N_OF[p.scene] != N_OF[st.scene]:
                return "size"
        elif p.gen != st.gen:
            return "stale"
    if call in DERIVATIVES and N_OF[st.scene] > 0 and st.opt[:2] not in SMOOTH:
        return "pair"
    return None


def qualifies64(st):
    """The float64 references apply: small enough for the oracle and the models, options the suites state their bounds for, plain lists"""
    return (1 <= N_OF[st.scene] <= 300 and st.bundle.count <= 130 and st.opt[2] in (1e-9, 0.0) and st.opt[:2] in MODELLED and not replayed(st))


# ---- the step generator ----
def _aim(scene):
    return scene if N_OF[scene] else "cloud-300"         # rays cannot aim at a scene of nothing


def walk(seed, n):
    """Yields ((op, call, how), state after the op, verdict of the call, stream turn): the whole sequence is a function of (seed, n)"""
    rng = np.random.default_rng(seed)
    st = State()
    turn = 0
    for _ in range(n):
        st = dataclasses.replace(st)
        stuck = st.plan is not None and verdict(st, "radiance") is not None      # a plan that refuses everything: mostly, do something about it
        ops = ("unplan", "plan", "plan-keep") if stuck and rng.random() < 0.85 else OPS
        op = str(rng.choice(ops, p=OP_P if ops is OPS else None))
        if op == "frame" and N_OF[st.scene] == 0:
            op = "none"
        if op == "scene":
            twin = st.scene[:-1] if st.scene.endswith("~") else st.scene + "~"
            if st.plan is not None and st.plan.keep and twin in N_OF and rng.random() < 0.7:
                st.scene = twin                                                    # the same N: the plan's lists stay in force
            else:
                others = [s for s in SCENES if s != st.scene]
                w = np.array([SCENE_WEIGHT.get(s, 1.0) for s in others])
                st.scene = str(rng.choice(others, p=w / w.sum()))
            st.setter = str(rng.choice(["host", "device", "side"]))
            st.gen += 1
            big = st.scene == WIDE and st.bundle.count > 130                       # a thousand rays of a thousand entries each: minutes of model
            if st.plan is None and (big or rng.random() < 0.5):
                st.bundle = Bundle(_aim(st.scene), 130 if big else st.bundle.count, st.bundle.per_ray, int(rng.integers(1000)))
        elif op == "bundle":
            same = st.plan is not None and rng.random() < 0.5                      # other rays of the plan's count: the plan's lists
            count = st.bundle.count if same else int(rng.choice(COUNTS))
            if st.scene == WIDE:
                count = min(count, 130)
            st.bundle = Bundle(_aim(st.scene), count, bool(rng.random() < 0.3), int(rng.integers(1000)))
        elif op == "options":
            opt = PAIRS[int(rng.integers(len(PAIRS)))] + (float(rng.choice(EPS)),)
            st.gen += opt != st.opt
            st.opt = opt
        elif op in ("index", "sort", "ordered", "stats"):
            setattr(st, op, not getattr(st, op))
        elif op in ("plan", "plan-keep"):
            st.plan = Plan(op == "plan-keep", st.scene, st.opt, st.bundle, st.gen)
        elif op == "unplan":
            st.plan = None
        calls = CALLS
        if st.opt[:2] not in SMOOTH and rng.random() < 0.7:
            calls = tuple(c for c in CALLS if c not in DERIVATIVES)                # under a pair with jumps: mostly what it can still do
        call = str(rng.choice(calls))
        how = str(rng.choice(HOWS, p=HOW_P))
        yield (op, call, how), st, verdict(st, call), turn
        turn += how != "host"


def steps(seed, n):
    """(op, call, how) triples"""
    for step, _, _, _ in walk(seed, n):
        yield step


# ---- scenes, rays and inputs: built once ----
_scenes, _rays, _inputs = {}, {}, {}


def scene(oracle, name):
    if name not in _scenes:
        if name.startswith("cloud"):
            n = N_OF[name]
            g = RS.cloud(oracle, n) if n else oracle.gaussians(np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(0), np.zeros(0))
            if name.endswith("~"):
                rng = np.random.default_rng(7300 + n)
                g = g.copy()
                g["mu"][:, :3] += (0.3 * g["sigma"][:, None] * rng.normal(size=(n, 3))).astype(np.float32)
                g["sigma"] *= rng.uniform(0.97, 1.03, n).astype(np.float32)
                g["albedo"] = np.clip(g["albedo"] + rng.uniform(-0.05, 0.05, size=(n, 4)), 0.0, 1.0).astype(np.float32)
        elif name == STACK:
            g = R.stack_with_side(oracle, RAY_PL + 1)
        else:
            g = R.wide_stack(oracle, RAY_LCAP, RAY_LCAP + 1).g
        _scenes[name] = np.ascontiguousarray(g)
    return _scenes[name]


def rays_of(oracle, b):
    """(origins [3] or [count, 3], dirs [count, 3]) float32: ray_sort_scenes.aimed_rays at the Gaussians of b.aim"""
    if b not in _rays:
        o, d = RS.aimed_rays(scene(oracle, b.aim), b.count, 50000 + b.seed, per_ray_origin=b.per_ray)
        o = np.ascontiguousarray(o, np.float32)
        _rays[b] = (o.reshape(3) if o.size == 3 else o, np.ascontiguousarray(d, np.float32))      # one ray's own origin is the bundle's
    return _rays[b]


def inputs(b, n_scene):
    """What the entry points take besides the rays, seeded by (bundle, scene size)"""
    key = (b, n_scene)
    if key not in _inputs:
        rng = np.random.default_rng([b.count, b.seed, n_scene, int(b.per_ray)])
        n, ns = b.count, len(SAMPLES)
        u = lambda *shape: rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)  # noqa: E731
        x = {"gr": u(n, 4), "gT": u(n, ns), "s_ray": (SAMPLES[None, :] + 0.2 * u(n, ns)).astype(np.float32), "tan": 0.1 * u(n_scene, 12),
             "rtan": 0.1 * u(n, 8), "stan": 0.1 * u(n, ns), "w": rng.uniform(0.25, 4.0, size=(n, 4)).astype(np.float32)}
        x["s3"], x["stan3"] = np.ascontiguousarray(x["s_ray"][:, :3]), np.ascontiguousarray(x["stan"][:, :3])
        _inputs[key] = x
    return _inputs[key]


def packed(g):
    """The four arrays the device setter takes"""
    return (np.ascontiguousarray(g["mu"][:, :3], np.float32), np.ascontiguousarray(g["albedo"], np.float32),
            np.ascontiguousarray(g["sigma"], np.float32), np.ascontiguousarray(g["magnitude"], np.float32))


# ---- what the model says of a step: list lengths, darkness (the CPU test's conditions) ----
_lens = {}


def lists_of(st):
    """(scene, options, bundle) whose cull gives the lists a call in st sums over: the plan's when one is bound"""
    p = st.plan
    return (p.scene, p.opt, p.bundle) if p is not None else (st.scene, st.opt, st.bundle)


def kept_lists(oracle, name, opt, b):
    """ray_bundle_scenes.kept per ray as index arrays, 128 rays at a time"""
    key = (name, opt[0], opt[2], b)
    if key not in _lens:
        g = scene(oracle, name)
        o, d = rays_of(oracle, b)
        ek = opt[0] if opt[0] in R.EXP_FLOOR else 1       # the Exp kinds without an entry flush no later than vcl_exp: a length, not a bit
        out = []
        for r0 in range(0, len(d), 128):
            keep = R.kept(o if o.size == 3 else o[r0:r0 + 128], d[r0:r0 + 128], g, opt[2], ek)
            out += [np.flatnonzero(k) for k in keep]
        _lens[key] = out
    return _lens[key]


def kernels_reached(oracle, st):
    """{"short", "long", "scratch"} of the rays of a call in st, from the float64 list lengths"""
    n = np.array([len(l) for l in kept_lists(oracle, *lists_of(st))])
    return {k for k, on in (("short", (n <= RAY_PL).any()), ("long", ((n > RAY_PL) & (n <= RAY_LCAP)).any()), ("scratch", (n > RAY_LCAP).any())) if on}


def list_source(st):
    return "plan" if st.plan is not None else "index" if st.index else "chunks"


def lit(oracle, st):
    """Some ray keeps a Gaussian and sees it: radiance > 0 or T < 1 by the oracle over its list, on the current scene"""
    lists = kept_lists(oracle, *lists_of(st))
    g = scene(oracle, st.scene)
    if not len(g) or st.opt[0] not in (0, 1) or st.opt[1] not in (0, 1):
        ek, fk = 1, 1
    else:
        ek, fk = st.opt[:2]
    o, d = rays_of(oracle, st.bundle)
    for r in np.argsort([-len(l) for l in lists], kind="stable")[:4]:
        idx = lists[r][lists[r] < len(g)]
        if len(idx):
            orig = o if o.size == 3 else o[r]
            if oracle.radiance(orig, d[r], g[idx], ek, fk).max() > 0 or (oracle.transmittance(orig, d[r], SAMPLES[-1:], g[idx], ek, fk) < 1).any():
                return True
    return False


# ---- the float64 references ----
class Reference:
    """The oracle's full sums and the gradient suites' float64 models for the steps that qualify (qualifies64), computed once each"""

    def __init__(self, oracle):
        self.O, self._c = oracle, {}

    def _cached(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def check(self, ctx, st):
        """Names of what ctx, a plain fresh context in state st, misses of the oracle's full sums"""
        import transmittance_bundle_scenes as TB
        O = self.O
        g, (o, d), (ek, fk, eps) = scene(O, st.scene), rays_of(O, st.bundle), st.opt
        key = (st.scene, st.bundle, st.opt)
        lo, hi = self._cached(("range",) + key, lambda: R.kept_range(o, d, g, eps, ek))
        ref = self._cached(("L",) + key[:2] + (ek, fk), lambda: R.oracle_radiance(O, o, d, g, ek, fk))
        refT = self._cached(("T",) + key[:2] + (ek, fk), lambda: TB.oracle_T(O, o, d, SAMPLES, g, ek, fk))
        rad = ctx.host("radiance", st.bundle)["radiance"]
        T = ctx.host("T shared", st.bundle)["T"]
        eL = np.abs(rad.astype(np.float64) - ref).max(1)
        eT = np.abs(T.astype(np.float64) - refT).max(1)
        bad = []
        if not (eL <= R.tolerance(lo, hi, float(ref.max()), nocull=eps == 0)).all():
            bad.append(f"radiance against the oracle: {eL.max():.3e}")
        if not (eT <= TB.tolerance(lo, hi, len(g), eps)).all():
            bad.append(f"T against the oracle: {eT.max():.3e}")
        return bad

    def table_bound(self, st, call):
        """What a float-atomic table may differ by from another summation order of the same call: twice the suites' bound, [N, columns];
        None where no bound is stated"""
        if call not in ("grad", "tgrad") or not qualifies64(st):
            return None
        import grad_bundle_scenes as G
        import trans_grad_bundle_scenes as T
        O = self.O
        g, (o, d), (ek, fk, eps) = scene(O, st.scene), rays_of(O, st.bundle), st.opt
        x = inputs(st.bundle, len(g))
        name = f"state {st.scene} {tuple(st.bundle)}"
        sc = G.GradScene(name, g, o, d, x["gr"], [])
        pair = MODELLED[(ek, fk)]
        if call == "grad":
            return 2 * G.bound(G.model(sc, pair, eps)[1])
        return self._cached(("tgrad", name, pair, eps), lambda: 2 * T.bound(T.bundle_tgrad(T.Case(name, sc, 0, x["s_ray"], x["gT"]), pair, eps).S))


# ---- the driver ----
class Refused(Exception):
    """A context refused a call with VRT_HIP_ERR_INVALID where `run` did not expect it to"""


def status_of(error):
    """The library's status in a VrtHipError ("<what> failed (<status>): <message>"); an error that does not carry one goes up as it is"""
    m = re.search(r"failed \((-?\d+)\)", str(error))
    if m is None:
        raise error
    return int(m.group(1))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(got, want, atomic=False, bound=None):
    """Names of the results that differ: bit for bit, but a float-atomic "table" within `bound` of the ordered one.  Without a bound
    what needs none is still held: the shape, the same entries finite, and exact zeros in the rows the ordered table leaves untouched
    (a Gaussian no ray keeps gets no add at all) -- a table written for another N or another list does not pass these."""
    bad = [k for k in want if k not in got]
    for k in want:
        if k not in got:
            continue
        if k == "table" and atomic:
            a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
            if a.shape != b.shape:
                bad.append("atomic table: shape")
            elif not np.array_equal(np.isfinite(a), np.isfinite(b)):
                bad.append("atomic table: other entries finite")
            elif (a[(b == 0).all(1)] != 0).any():
                bad.append("atomic table: a row no ray keeps was written")
            elif bound is not None and not (np.abs(a - b) <= bound).all():
                bad.append("atomic table beyond the bound")
        elif not same_bits(got[k], want[k]):
            bad.append(k)
    return bad


def plain(ctx, st):
    """A fresh context's switches: index off, sort off, ordered on, statistics on"""
    ctx.set_switch("index", False)
    ctx.set_switch("sort", False)
    ctx.set_switch("ordered", True)
    ctx.set_switch("stats", True)


def expectation(make_fresh, st, refused):
    """A fresh context that computes what the call of this step must give: plain, unless the bound plan's lists are not the plain
    ones (replayed) or the call must be refused -- then it goes the way A went: the plan's state, the plan, the current state"""
    B = make_fresh()
    plain(B, st)
    p = st.plan
    if p is not None and (refused or replayed(st)):
        B.set_scene(p.scene, "host", 0)
        B.set_options(p.opt)
        B.make_plan(p.bundle, p.keep)
        if refused or p.scene != st.scene:
            B.set_scene(st.scene, "host", 0)
        B.set_options(st.opt)
    else:
        B.set_scene(st.scene, "host", 0)
        B.set_options(st.opt)
    return B


def launched(st, call):
    """A derivative of a scene of no Gaussians launches nothing and reports nothing: statistics, records and order stay an earlier call's"""
    return N_OF[st.scene] > 0 or call not in DERIVATIVES


def expected(make_fresh, step, st, why, reference=None):
    """Everything a step is held to, from fresh contexts alone: the new plan's lists, the frame, the refusal's code or the call's results,
    statistics, records, order, the atomic table's bound, and what the fresh context itself misses of the float64 references"""
    op, call, how = step
    E = {"found": []}
    B = None
    if op in ("plan", "plan-keep"):
        B = expectation(make_fresh, dataclasses.replace(st, plan=None), False)
        B.make_plan(st.bundle, st.plan.keep)
        E["plan lists"] = B.plan_lists()
        B.unplan()                                                            # a plan just made is the plain cull: B goes on as the plain context
    elif op == "frame":
        B = expectation(make_fresh, dataclasses.replace(st, plan=None), False)
        E["frame"] = B.frame()
    if B is not None and (why or replayed(st)):
        B.close()
        B = None
    if B is None:
        B = expectation(make_fresh, st, bool(why))
    if why:
        E["code"] = B.host_code(call, st.bundle)
    else:
        E["want"] = B.host(call, st.bundle)
        E["atomic"] = call in TABLES and not st.ordered
        E["bound"] = reference.table_bound(st, call) if (reference is not None and E["atomic"]) else None
        E["stats"] = B.stats()
        if call in TABLES and launched(st, call):
            E["records"] = B.records()
        if st.sort and st.plan is None and st.bundle.count > 64 and launched(st, call):
            B.set_switch("index", st.index)
            B.set_switch("sort", True)
            B.host("radiance", st.bundle)
            E["order"] = B.order()
            B.set_switch("index", False)
            B.set_switch("sort", False)
        if reference is not None and qualifies64(st):
            E["found"] += reference.check(B, st)
    B.close()
    return E


def run(A, make_fresh, seed, n, reference=None, out=None):
    """Applies steps(seed, n) to the long-lived context A and holds every step to fresh contexts of make_fresh().  A and the fresh ones
    speak the small interface of `Gpu` (and of the CPU test's stub).  Returns the list of mismatches, one line each.
    The expectations of ALL steps are computed first: making, using and closing a fresh context waits for the whole device, and between
    a nosync bundle and the next step's state change -- or the next bundle, on another stream -- nothing but the library may wait."""
    bad, pending = [], None
    say = out or (lambda *_: None)
    sequence = list(walk(seed, n))
    wants = [expected(make_fresh, step, st, why, reference) for step, st, why, _ in sequence]
    first = State()
    for sw in ("index", "sort", "ordered", "stats"):
        A.set_switch(sw, False)
    A.set_scene(first.scene, "host", 0)
    A.set_options(first.opt)

    def judge(op):
        nonlocal pending
        if pending is not None:
            ticket, E, at = pending
            pending = None
            running = A.running(ticket) if hasattr(A, "running") else None   # a figure for the log, never a condition: it depends on timing
            late = differing(A.collect(ticket), E["want"], E["atomic"], E["bound"])
            if late:
                bad.append(f"step {at}: left in flight across '{op}': {late}")
            say(f"        step {at} left in flight across '{op}'{' (still running behind it)' if running else ''}: "
                f"{'ok' if not late else 'MISMATCH  <-- FAIL ' + str(late)}")

    for i, (((op, call, how), st, why, turn), E) in enumerate(zip(sequence, wants)):
        found = list(E["found"])
        # the state change, with the bundle of a nosync step before it still in flight
        if op == "scene":
            A.set_scene(st.scene, st.setter, turn + 1)
        elif op == "options":
            A.set_options(st.opt)
        elif op in ("index", "sort", "ordered", "stats"):
            A.set_switch(op, getattr(st, op))
        elif op in ("plan", "plan-keep"):
            A.unplan()
            A.make_plan(st.bundle, st.plan.keep)
        elif op == "unplan":
            A.unplan()
        elif op == "frame":
            if not same_bits(A.frame(), E["frame"]):
                found.append("frame")
        if op in ("plan", "plan-keep") and not same_bits(A.plan_lists(), E["plan lists"]):
            found.append("plan lists")
        if why:
            # refused by both, with the same code, before anything is written
            judge(op)
            code_a, untouched = A.refused(call, st.bundle, turn)
            if how == "host":
                code_a = min(code_a, A.host_code(call, st.bundle))
            if not (code_a == E["code"] == INVALID):
                found.append(f"refusal ({why}): codes {code_a} and {E['code']}")
            if not untouched:
                found.append(f"refusal ({why}): an output was written")
        else:
            got = None
            try:
                if how == "host":
                    judge(op)
                    got = A.host(call, st.bundle)
                else:
                    # enqueued BEFORE the bundle in flight is waited for: on another stream, the library alone orders the two
                    ticket = A.enqueue(call, st.bundle, turn, 1 if how == "device" else 3)
                    judge(op)
                    if how == "nosync":
                        pending = (ticket, E, i)
                    else:
                        got = A.collect(ticket)
            except Refused as e:
                judge(op)
                found.append(f"refused a call it must admit: {e}")
            if got is not None:
                found += differing(got, E["want"], E["atomic"], E["bound"])
                if st.stats and launched(st, call) and not same_bits(A.stats(), E["stats"]):
                    found.append(f"ray_stats {A.stats()} != {E['stats']}")
                if st.ordered and "records" in E:
                    rec = A.records()
                    if differing(rec, E["records"]):
                        found.append("grad_records")
                    if int(rec["mismatches"][0]) != 0:
                        found.append("ordered mismatches")
                if "order" in E:
                    A_order = A.order()
                    if A_order is None or not same_bits(A_order, E["order"]):
                        found.append("ray_order")
        if found:
            bad.append(f"step {i}: {found}")
        say(f"step {i}: {op:9s} -> {st.scene} by {st.setter}, {st.bundle.count} rays{' (own origins)' if st.bundle.per_ray else ''} opt={st.opt} "
            f"index={int(st.index)} sort={int(st.sort)} ordered={int(st.ordered)} stats={int(st.stats)} "
            f"plan={'none' if st.plan is None else ('keep' if st.plan.keep else 'strict') + (' replayed' if replayed(st) else '')}: {call} via {how}"
            f"{' refused (' + why + ')' if why else ''}: {'ok' if not found else 'MISMATCH  <-- FAIL ' + str(found)}")
    judge("the end")
    A.unplan()
    return bad


# ---- the interface over a real context ----
POISON = 0x5A5A5A5A


class Gpu:
    """The interface `run` speaks, over Renderer: set_scene, set_options, set_switch, make_plan, unplan, plan_lists, frame, host,
    host_code, enqueue, collect, refused, stats, records, order, close"""
    _streams = None
    _scenes = {}                 # the device setter's arrays of every scene, staged once and never freed: work in flight may read them

    def __init__(self, pkg, oracle, renderer=None):
        import torch
        self.pkg, self.O, self.torch = pkg, oracle, torch
        self.r = renderer if renderer is not None else pkg.Renderer(0)
        self.plan = None
        if Gpu._streams is None:
            Gpu._streams = [torch.cuda.Stream() for _ in range(NSTREAMS)]
            for name in SCENES:
                Gpu._scenes[name] = [self.cuda(a) for a in packed(scene(oracle, name))]
            torch.cuda.synchronize()

    def wait_for_staging(self):
        """Waits for torch's current stream, where inputs were copied and outputs filled -- NOT for the device: a bundle of this context
        may be in flight on another stream, and only the library may order anything against it"""
        self.torch.cuda.current_stream().synchronize()

    def stream(self, turn):
        return Gpu._streams[turn % NSTREAMS]

    def cuda(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def close(self):
        self.unplan()
        self.torch.cuda.synchronize()
        self.r.close()

    # -- state --
    def set_scene(self, name, how, turn):
        g = scene(self.O, name)
        if how == "host":
            self.r.set_gaussians(g)
            return
        t = Gpu._scenes[name]                             # staged long ago: nothing is copied and nothing waited for here
        self.r.set_gaussians_device(len(g), *[a.data_ptr() for a in t], stream=0 if how == "device" else self.stream(turn).cuda_stream)

    def set_options(self, opt):
        self.r.set_options(*opt)

    def set_switch(self, name, on):
        {"index": self.r.set_ray_index, "sort": self.r.set_ray_sort, "ordered": self.r.set_grad_ordered, "stats": self.r.enable_stats}[name](on)

    def make_plan(self, b, keep):
        self.plan = self.r.ray_plan(*rays_of(self.O, b))
        self.r.set_ray_plan(self.plan, keep_lists=keep)

    def unplan(self):
        self.r.set_ray_plan(None)
        if self.plan is not None:
            self.plan.close()
            self.plan = None

    def plan_lists(self):
        offsets, entries = self.plan.lists()
        return np.concatenate([offsets, entries.astype(np.uint64)])

    def frame(self, w=32, h=32, tiles=4):
        O, torch = self.O, self.torch
        cam, _ = O.cli_camera(w, h, camera_offset=-4.0)
        view = O.camera_view(cam)
        self.r.set_camera_view(w, h, view)
        out = torch.zeros(w * h, dtype=torch.int32, device="cuda")           # cleared on torch's current stream, the one the frame runs on
        self.r.frame_call(2.0 / tiles, 2.0 / tiles, view, np.array(cam.position[:], np.float32), self.pkg.PACK_ROUND | self.pkg.ALPHA_COMPUTED)(
            out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return out.cpu().numpy().view(np.uint32)                              # waits for that stream alone

    def _admitted(self, fn, *args):
        """fn(*args); a VRT_HIP_ERR_INVALID as Refused (every other error is the library's failure and goes up as it is)"""
        try:
            return fn(*args)
        except self.pkg.VrtHipError as e:
            if status_of(e) == INVALID:
                raise Refused(str(e)) from None
            raise

    # -- host forms --
    def host(self, call, b):
        return self._admitted(self._host, call, b)

    def _host(self, call, b):
        r = self.r
        o, d = rays_of(self.O, b)
        x = inputs(b, r.n)
        if call == "radiance":
            rad, img = r.radiance_rays(o, d, want_image=True)
            return {"radiance": rad, "pixels": img}
        if call == "T shared":
            return {"T": r.transmittance_bundle(o, d, SAMPLES)}
        if call == "T per ray":
            return {"T": r.transmittance_bundle(o, d, x["s_ray"])}
        if call == "depth":
            return {"depth": r.depth_bundle(o, d, LEVELS)}
        if call == "grad":
            t, rows = r.radiance_rays_grad(o, d, x["gr"], want_rays=True)
            table = np.concatenate([t["albedo"], t["mu"], t["sigma"][:, None], t["magnitude"][:, None]], 1)
            return {"table": table, "rows origin": rows["origin"], "rows dir": rows["dir"]}
        if call == "tgrad":
            t, gs, rows = r.transmittance_bundle_grad(o, d, x["s_ray"], x["gT"], want_rays=True)
            table = np.concatenate([t["mu"], t["sigma"][:, None], t["magnitude"][:, None]], 1)
            return {"table": table, "grad_s": gs, "rows origin": rows["origin"], "rows dir": rows["dir"]}
        if call == "tangent":
            return {"out": r.radiance_rays_tangent(o, d, x["tan"], x["rtan"])}
        if call == "ttangent T":
            return {"out": r.transmittance_bundle_tangent(o, d, x["s_ray"], x["tan"], x["rtan"], x["stan"])}
        if call == "ttangent depth":
            depth = r.depth_bundle(o, d, LEVELS)
            return {"depth": depth, "out": r.transmittance_bundle_tangent(o, d, depth, x["tan"], x["rtan"], x["stan3"], wrt=self.pkg.TGRAD_DEPTH, s_per_ray=True)}
        assert call == "gn_diag", call
        return {"table": np.ascontiguousarray(r.radiance_rays_gn_diag(o, d, x["w"])[:, :9])}

    def host_code(self, call, b):
        """The status of the host form: 0, or the code of the error it raises"""
        try:
            self._host(call, b)
        except self.pkg.VrtHipError as e:
            return status_of(e)
        return 0

    # -- device forms --
    def _outputs(self, call, b, fill):
        torch, n, N, ns = self.torch, b.count, self.r.n, len(SAMPLES)
        shapes = {"radiance": {"radiance": (n, 4), "pixels": (n,)}, "T shared": {"T": (n, ns)}, "T per ray": {"T": (n, ns)}, "depth": {"depth": (n, 3)},
                  "grad": {"table": (N, 12), "rows": (n, 8)}, "tgrad": {"table": (N, 12), "grad_s": (n, ns), "rows": (n, 8)},
                  "tangent": {"out": (n, 4)}, "ttangent T": {"out": (n, ns)}, "ttangent depth": {"depth": (n, 3), "out": (n, 3)},
                  "gn_diag": {"table": (N, 12)}}[call]
        return {k: torch.full(s, fill, dtype=torch.int32, device="cuda") for k, s in shapes.items()}

    def _launch(self, call, b, t, out, stream, depths_given=False):
        r, n, ns = self.r, b.count, len(SAMPLES)
        per_ray = t["o"].numel() != 3
        rays = (n, t["o"].data_ptr(), per_ray, t["d"].data_ptr())
        p = lambda k: (out[k] if k in out else t[k]).data_ptr()  # noqa: E731
        if call == "radiance":
            r.radiance_rays_device(*rays, d_radiance=p("radiance"), d_image=p("pixels"), stream=stream)
        elif call == "T shared":
            r.transmittance_bundle_device(*rays, p("samples"), ns, False, p("T"), stream=stream)
        elif call == "T per ray":
            r.transmittance_bundle_device(*rays, p("s_ray"), ns, True, p("T"), stream=stream)
        elif call == "depth":
            r.depth_bundle_device(*rays, p("levels"), 3, False, p("depth"), stream=stream)
        elif call == "grad":
            r.radiance_rays_grad_rays_device(*rays, p("gr"), d_grad=p("table"), d_grad_rays=p("rows"), stream=stream)
        elif call == "tgrad":
            r.transmittance_bundle_grad_rays_device(*rays, p("s_ray"), ns, True, p("gT"), self.pkg.TGRAD_T, d_grad=p("table"), d_grad_s=p("grad_s"),
                                                    d_grad_rays=p("rows"), stream=stream)
        elif call == "tangent":
            r.radiance_rays_tangent_device(*rays, d_tangent=p("tan"), d_ray_tangent=p("rtan"), d_out=p("out"), stream=stream)
        elif call == "ttangent T":
            r.transmittance_bundle_tangent_device(*rays, p("s_ray"), ns, True, self.pkg.TGRAD_T, d_tangent=p("tan"), d_ray_tangent=p("rtan"),
                                                  d_s_tangent=p("stan"), s_tangent_per_ray=True, d_out=p("out"), stream=stream)
        elif call == "ttangent depth":
            if not depths_given:
                r.depth_bundle_device(*rays, p("levels"), 3, False, p("depth"), stream=stream)
            r.transmittance_bundle_tangent_device(*rays, p("s3") if depths_given else p("depth"), 3, True, self.pkg.TGRAD_DEPTH, d_tangent=p("tan"),
                                                  d_ray_tangent=p("rtan"), d_s_tangent=p("stan3"), s_tangent_per_ray=True, d_out=p("out"), stream=stream)
        else:
            r.radiance_rays_gn_diag_device(*rays, d_weights=p("w"), d_diag=p("table"), stream=stream)

    def _staged(self, b):
        o, d = rays_of(self.O, b)
        t = {k: self.cuda(v) for k, v in inputs(b, self.r.n).items()}
        t.update(o=self.cuda(o), d=self.cuda(d), samples=self.cuda(SAMPLES), levels=self.cuda(LEVELS))
        return t

    def enqueue(self, call, b, turn, reps):
        """`reps` device calls back to back on one of the three streams, nothing waited for; the ticket of the last one"""
        t = self._staged(b)
        outs = [self._outputs(call, b, 0) for _ in range(reps)]
        self.wait_for_staging()                           # inputs and cleared outputs are there
        st = self.stream(turn)
        for out in outs:
            self._admitted(self._launch, call, b, t, out, st.cuda_stream)
        return (call, t, outs, st)

    def running(self, ticket):
        """The ticket's stream has not finished yet (asks, does not wait)"""
        return not ticket[3].query()

    def collect(self, ticket):
        call, t, outs, st = ticket
        st.synchronize()                                  # the ticket's stream alone: a later bundle on another stream stays in flight
        res = {k: v.cpu().numpy() for k, v in outs[-1].items()}
        f32 = lambda a: a.view(np.float32)  # noqa: E731
        if call == "radiance":
            return {"radiance": f32(res["radiance"]), "pixels": res["pixels"].view(np.uint32)}
        got = {k: f32(v) for k, v in res.items() if k not in ("table", "rows")}
        if "table" in res:
            got["table"] = np.ascontiguousarray(f32(res["table"])[:, 4:9] if call == "tgrad" else f32(res["table"])[:, :9])
        if "rows" in res:
            got["rows origin"], got["rows dir"] = f32(res["rows"])[:, 0:3], f32(res["rows"])[:, 4:7]
        return got

    def refused(self, call, b, turn):
        """The device form over outputs filled with a pattern: (its status, every output word still the pattern)"""
        t = self._staged(b)
        out = self._outputs(call, b, POISON)
        self.wait_for_staging()
        code = 0
        try:
            self._launch(call, b, t, out, self.stream(turn).cuda_stream, depths_given=True)
        except self.pkg.VrtHipError as e:
            code = status_of(e)
        self.torch.cuda.synchronize()
        return code, all(bool((v == POISON).all()) for v in out.values())

    # -- what the library reports of the last bundle --
    def stats(self):
        s = self.r.ray_stats()
        return np.array([s[k] for k in SAME_STATS], np.uint64)

    def records(self):
        gauss, ray, rows = self.r.grad_records()
        return {"gauss": gauss, "ray": ray, "rows": rows, "mismatches": np.array([self.r.grad_ordered_stats()["mismatches"], 0], np.uint64)}

    def order(self):
        if not self.r.ray_sort_stats()["sorted"]:
            return None
        order, keys = self.r.ray_order()
        return np.concatenate([order, keys])


def main(argv):
    sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
    from conftest import load_pkg
    pkg = load_pkg()
    import oracle as O
    O.build()
    seed = int(argv[1]) if len(argv) > 1 else 0
    nsteps = int(argv[2]) if len(argv) > 2 else 100
    A = Gpu(pkg, O)
    bad = run(A, lambda: Gpu(pkg, O), seed, nsteps, Reference(O), out=lambda line: print(line, flush=True))
    A.close()
    for line in bad:
        print(line)
    print("mismatches:", len(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
