"""Ordered gradient tables on the GPU (vrt_hip_set_grad_ordered, csrc/vrt_grad_ordered_kernel.hip and the ORDERED instantiations of the
four gradient kernels).  The table is held BIT FOR BIT to tests/grad_ordered_scenes.ordered_reduce of the call's own records
(vrt_hip_get_grad_records), the records to the float64 models of grad_bundle_scenes / trans_grad_bundle_scenes within the project's
B = RHO * S, and everything else an ordered call returns to the atomic call's bits."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import grad_bundle_scenes as G
import grad_ordered_scenes as O
import trans_grad_bundle_scenes as T
from grad_bundle_scenes import PAIRS, RAY_LCAP, RAY_PL
from trans_grad_bundle_scenes import TGRAD_T

pytestmark = pytest.mark.gpu

bits = O.bits


@contextlib.contextmanager
def ordered(renderer, on=True):
    renderer.set_grad_ordered(on)
    try:
        yield renderer
    finally:
        renderer.set_grad_ordered(False)


def setup(renderer, g, pair="vcl-as", eps=1e-9):
    renderer.set_options(*PAIRS[pair], eps)
    renderer.set_gaussians(g)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Radiance:
    """A radiance gradient bundle of a GradScene through the device form"""
    cols, two = O.RADIANCE_COLS, True

    def __init__(self, sc):
        self.sc, self.n, self.nrays = sc, len(sc.g), len(sc.d)
        self.per = int(sc.o.size != 3)
        self.t = [cuda(a) for a in (sc.o, sc.d, sc.gr)]

    def device(self, renderer, table, rows=None, gs=None, stream=0):
        renderer.radiance_rays_grad_rays_device(self.nrays, self.t[0].data_ptr(), self.per, self.t[1].data_ptr(), self.t[2].data_ptr(),
                                                table.data_ptr() if table is not None else 0, rows.data_ptr() if rows is not None else 0, stream)

    def host(self, renderer):
        """(table [N, 12] float32, None, ray rows) of the host form"""
        n = self.n
        out, rows = np.full((n, O.STRIDE), 7.0, np.float32), np.zeros((self.nrays, 8), np.float32)
        f32p = C.POINTER(C.c_float)
        o, d, g = (np.ascontiguousarray(a, np.float32) for a in (self.sc.o, self.sc.d, self.sc.gr))
        rc = renderer._L.vrt_hip_radiance_rays_grad_rays(renderer._h, self.nrays, o.ctypes.data_as(f32p), self.per, d.ctypes.data_as(f32p),
                                                         g.ctypes.data_as(f32p), out.ctypes.data_as(f32p), rows.ctypes.data_as(f32p))
        renderer._chk(rc, "radiance_rays_grad_rays")
        return out, None, rows

    def lens(self, eps, pair):
        return [len(l) for l in self.sc.lists(eps, PAIRS[pair][0])]

    def model(self, pair, eps):
        key = (self.sc.name, pair, eps)
        if key not in _MODELS:
            _MODELS[key] = G.model(self.sc, pair, eps) if self.sc.name in _SUITE else G.bundle_grad(self.sc, pair, eps)[:2]
        return _MODELS[key]

    bound = staticmethod(G.bound)


class Trans:
    """A transmittance gradient bundle of a Case through the device form, at the samples s (depth mode: the depths of this context)"""
    cols, two = O.TRANS_COLS, False

    def __init__(self, case, s):
        sc = case.sc
        self.case, self.sc, self.s, self.n, self.nrays = case, sc, np.ascontiguousarray(s, np.float32), len(sc.g), len(sc.d)
        self.per, self.s_per_ray, self.ns = int(sc.o.size != 3), int(self.s.ndim == 2), self.s.shape[-1]
        self.t = [cuda(a) for a in (sc.o, sc.d, self.s, case.g)]

    def device(self, renderer, table, rows=None, gs=None, stream=0):
        p = [a.data_ptr() for a in self.t]
        renderer.transmittance_bundle_grad_rays_device(self.nrays, p[0], self.per, p[1], p[2], self.ns, self.s_per_ray, p[3], self.case.wrt,
                                                       table.data_ptr() if table is not None else 0, gs.data_ptr() if gs is not None else 0,
                                                       rows.data_ptr() if rows is not None else 0, stream)

    def host(self, renderer):
        grad, gs, rows = renderer.transmittance_bundle_grad(self.sc.o, self.sc.d, self.s, self.case.g, wrt=self.case.wrt, s_per_ray=bool(self.s_per_ray),
                                                            want_rays=True)
        out = np.zeros((self.n, O.STRIDE), np.float32)
        out[:, 0:4], out[:, 4:7], out[:, 7], out[:, 8] = grad["albedo"], grad["mu"], grad["sigma"], grad["magnitude"]
        return out, gs, np.concatenate([rows["origin"], np.zeros((self.nrays, 1), np.float32), rows["dir"], np.zeros((self.nrays, 1), np.float32)], 1)

    def lens(self, eps, pair):
        return [len(l) for l in self.sc.lists(eps, PAIRS[pair][0])]

    def model(self, pair, eps):
        m = T.bundle_tgrad(self.case, pair, eps, s=self.s)
        val, S = np.zeros((self.n, 9)), np.zeros((self.n, 9))
        val[:, 4:], S[:, 4:] = m.val, m.S
        return val, S

    bound = staticmethod(T.bound)


_MODELS = {}
_SUITE = set([f"small {n}" for n in (1, 2, 3, 4, 5, 9)] + [f"stack {k}|{k + 1}" for k in (RAY_PL, 64, 128)] + [f"wide {RAY_LCAP + 1}"]
             + ["grid16 coherent", "grid16 scattered"])


def samples(renderer, case):
    """The samples of a transmittance case as the device gets them: its own in T mode, what depth_bundle returns for its levels in depth mode"""
    if case.wrt == TGRAD_T:
        return case.s
    return renderer.depth_bundle(case.sc.o, case.sc.d, case.tau, True)


def call(renderer, b, table0=None, want_rows=False, want_gs=False, stream=None):
    """One device-form call into a copy of table0 (zeros without): (table [N, 12], ray rows or None, grad_s or None) as numpy arrays"""
    import torch
    table = torch.zeros((b.n, O.STRIDE), dtype=torch.float32, device="cuda") if table0 is None else cuda(table0)
    rows = cuda(np.full((b.nrays, 8), np.nan, np.float32)) if want_rows else None
    gs = cuda(np.full((b.nrays, b.ns), np.nan, np.float32)) if want_gs else None
    torch.cuda.synchronize()
    if stream is None:
        b.device(renderer, table, rows, gs)
    else:
        with torch.cuda.stream(stream):
            b.device(renderer, table, rows, gs, stream=stream.cuda_stream)
        stream.synchronize()
    renderer.sync()
    return table.cpu().numpy(), (rows.cpu().numpy() if want_rows else None), (gs.cpu().numpy() if want_gs else None)


def bundle_of(renderer, oracle, kind, name, pair="vcl-as", eps=1e-9):
    """The scene set, and the bundle of it: kind "rad" (a GradScene by name) or "T" / "depth" (a transmittance case by name)"""
    if kind == "rad":
        sc = O.bundle(oracle, name)
        setup(renderer, sc.g, pair, eps)
        return Radiance(sc)
    case = T.case(oracle, f"{kind} {name}")
    setup(renderer, case.sc.g, pair, eps)
    return Trans(case, samples(renderer, case))


def check_records(b, gauss, ray, rows, stats, eps=1e-9, pair="vcl-as"):
    """The records are in consumed order, as many as the model lists say, per Gaussian and ray as many as the ray's kind files"""
    key = (gauss.astype(np.int64) << 32) | ray.astype(np.int64)
    assert (np.diff(key) >= 0).all()                                    # (Gaussian, ray id); a ray's places keep their order (stable sort)
    lens = b.lens(eps, pair)
    assert len(gauss) == O.record_count(lens, b.two)
    per = np.zeros((b.n, b.nrays), np.int64)
    np.add.at(per, (gauss, ray), 1)
    want = np.zeros((b.n, b.nrays), np.int64)
    for r, idx in enumerate(b.sc.lists(eps, PAIRS[pair][0])):
        want[idx, r] = 2 if (b.two and len(idx) > RAY_PL) else 1
    assert (per == want).all()
    seg = np.bincount(gauss, minlength=b.n)
    assert stats == {"records": len(gauss), "gaussians": int((seg > 0).sum()), "longest": int(seg.max()) if len(gauss) else 0, "mismatches": 0}
    assert rows.shape == (len(gauss), 9) and np.isfinite(rows).all()
    if not b.two:
        assert (bits(rows[:, :4]) == 0).all()                           # columns nobody computes: +0


def bit_for_bit(renderer, b, wrong_must_show=False):
    n = b.n
    with ordered(renderer):
        first, _, _ = call(renderer, b)
        gauss, ray, rows = renderer.grad_records()
        stats = renderer.grad_ordered_stats()
        t0 = O.poison(O.random_table(n), O.written_cells(n, gauss, b.cols))
        got, _, _ = call(renderer, b, t0)
        again = renderer.grad_records()
    for a, c in zip((gauss, ray, rows), again):
        assert (bits(a) == bits(c)).all() if a.dtype == np.float32 else (a == c).all()
    check_records(b, gauss, ray, rows, stats)
    want = O.ordered_reduce(gauss, rows, t0, b.cols)
    assert (bits(got) == bits(want)).all(), np.argwhere(bits(got) != bits(want))[:4]      # all 12 N words: unwritten cells keep -0.0 and NaN payloads
    w = O.written_cells(n, gauss, b.cols)
    assert w.any() and (bits(got)[~w] == bits(t0)[~w]).all()
    assert (bits(first) == bits(O.ordered_reduce(gauss, rows, np.zeros((n, O.STRIDE), np.float32), b.cols))).all()
    if wrong_must_show:
        differ = [v for v in O.WRONG if (bits(O.ordered_reduce(gauss, rows, t0, b.cols, variant=v)) != bits(got)).any()]
        assert differ, "no wrong order shows on this bundle: it is too small to check the order"
    return gauss, ray, rows


RADIANCE = ["small 1", "small 5", "small 9", f"stack {RAY_PL}|{RAY_PL + 1}", f"wide {RAY_LCAP + 1}", "grid16 scattered"] + \
    [f"rays {k}" for k in O.K_RAYS] + ["aimed 64x64"]
TRANS = ["small 9 ns=1", "small 9 ns=5", f"stack {RAY_PL}|{RAY_PL + 1} ns={T.NSC + 1}", f"wide {RAY_LCAP + 1}"]


# ---- bit for bit against the model ----
@pytest.mark.parametrize("name", RADIANCE)
def test_radiance_table_is_the_ordered_sum_of_its_records(renderer, oracle, name):
    b = bundle_of(renderer, oracle, "rad", name)
    gauss, _, _ = bit_for_bit(renderer, b, wrong_must_show=name.startswith("aimed"))
    if name.startswith("rays"):
        assert (gauss == 1).all() and len(gauss) == int(name.split()[1])            # one segment of exactly k records
    if name.startswith("stack"):
        assert sorted(b.lens(1e-9, "vcl-as")) == [RAY_PL, RAY_PL + 1]                # one ray either side: both kernels recorded


@pytest.mark.parametrize("mode", ["T", "depth"])
@pytest.mark.parametrize("name", TRANS)
def test_transmittance_table_is_the_ordered_sum_of_its_records(renderer, oracle, name, mode):
    b = bundle_of(renderer, oracle, mode, name)
    bit_for_bit(renderer, b)


# ---- reproducibility ----
REPRO = [("rad", "aimed 64x64"), ("rad", f"stack {RAY_PL}|{RAY_PL + 1}"), ("rad", "grid16 scattered"), ("T", f"stack {RAY_PL}|{RAY_PL + 1} ns={T.NSC + 1}"),
         ("depth", "small 9 ns=5")]


@pytest.mark.parametrize("kind,name", REPRO)
def test_every_way_of_asking_gives_the_same_bits(renderer, oracle, kind, name):
    import torch
    b = bundle_of(renderer, oracle, kind, name)
    with ordered(renderer):
        ref, _, _ = call(renderer, b)
        assert np.abs(ref).max() > 0
        for _ in range(2):                                              # three runs
            assert (bits(call(renderer, b)[0]) == bits(ref)).all()
        renderer.set_ray_index(True)                                    # Morton index on
        try:
            assert (bits(call(renderer, b)[0]) == bits(ref)).all()
        finally:
            renderer.set_ray_index(False)
        host, _, _ = b.host(renderer)                                   # the host form against the device form onto a zero table
        assert (bits(host) == bits(ref)).all()
        renderer.enable_stats(True)                                     # statistics on
        try:
            assert (bits(call(renderer, b)[0]) == bits(ref)).all()
        finally:
            renderer.enable_stats(False)
        with_rows, rows, gs = call(renderer, b, want_rows=True, want_gs=kind != "rad")      # with ray rows (and grad_s)
        assert (bits(with_rows) == bits(ref)).all() and np.isfinite(rows).all()
        other, _, _ = call(renderer, b, stream=torch.cuda.Stream())    # another stream
        assert (bits(other) == bits(ref)).all()
    # ---- what an ordered call leaves as it was: ray rows and grad_s are the atomic call's, bit for bit ----
    _, rows_atomic, gs_atomic = call(renderer, b, want_rows=True, want_gs=kind != "rad")
    assert (bits(rows) == bits(rows_atomic)).all()
    if kind != "rad":
        assert (bits(gs) == bits(gs_atomic)).all()


# ---- statistics: an ordered call's are the atomic call's, field for field ----
@pytest.mark.parametrize("index", [False, True])
@pytest.mark.parametrize("kind,name", [("rad", "grid16 scattered"), ("rad", f"wide {RAY_LCAP + 1}"), ("T", f"stack {RAY_PL}|{RAY_PL + 1} ns={T.NSC + 1}")])
def test_ray_statistics_are_the_atomic_calls(renderer, oracle, kind, name, index):
    b = bundle_of(renderer, oracle, kind, name)
    renderer.set_ray_index(index)
    renderer.enable_stats(True)
    try:
        call(renderer, b)
        want = (renderer.ray_stats(), renderer.ray_index_stats())
        with ordered(renderer):
            call(renderer, b)
            got = (renderer.ray_stats(), renderer.ray_index_stats())
            assert renderer.grad_ordered_stats()["records"] > 0
    finally:
        renderer.enable_stats(False)
        renderer.set_ray_index(False)
    assert got == want and want[0]["rays"] == b.nrays


# ---- parity with the float64 models, within the project's own bound ----
def within(got, val, Ssum, bound, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    excess = np.abs(got - val) - bound(Ssum)
    j = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[j] <= 0, (what, j, got[j], val[j], bound(Ssum)[j])


PARITY = [("rad", n) for n in ("small 1", "small 5", "small 9", f"stack {RAY_PL}|{RAY_PL + 1}", f"wide {RAY_LCAP + 1}", "grid16 scattered", "rays 65",
                               "rays 129", "aimed 64x64")] + [(m, n) for m in ("T", "depth") for n in TRANS]


@pytest.mark.parametrize("eps", G.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("kind,name", PARITY)
def test_parity(renderer, oracle, kind, name, pair, eps):
    b = bundle_of(renderer, oracle, kind, name, pair, eps)
    with ordered(renderer):
        got, _, _ = call(renderer, b)
        stats = renderer.grad_ordered_stats()
    val, Ssum = b.model(pair, eps)
    within(got[:, :9], val, Ssum, b.bound, (kind, name, pair, eps))
    assert (got[:, 9:] == 0).all()
    assert stats["mismatches"] == 0 and stats["records"] == O.record_count(b.lens(eps, pair), b.two)
    # the next call with the switch off is the atomic path, and stays within the same bound
    atomic, _, _ = call(renderer, b)
    within(atomic[:, :9], val, Ssum, b.bound, (kind, name, pair, eps, "switch off again"))


# ---- edges ----
def test_nothing_to_do(renderer, oracle):
    import torch
    b = bundle_of(renderer, oracle, "rad", "rays 65")      # one Gaussian ahead of the origin and two far to the sides: a ray along x keeps none
    pattern = np.full((b.n, O.STRIDE), 0x7FC12345, np.uint32).view(np.float32)
    with ordered(renderer):
        call(renderer, b)
        assert renderer.grad_ordered_stats()["records"] > 0
        # 0 rays: nothing launched, the table untouched
        table = cuda(pattern)
        torch.cuda.synchronize()
        renderer.radiance_rays_grad_rays_device(0, b.t[0].data_ptr(), 0, b.t[1].data_ptr(), b.t[2].data_ptr(), table.data_ptr(), 0, 0)
        renderer.sync()
        assert (bits(table.cpu().numpy()) == 0x7FC12345).all()
        # every ray misses: 0 records, the table untouched, ray rows of exact zeros
        away = G.GradScene("away", b.sc.g, b.sc.o, np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (70, 1)), G.seeded_gr(70, 1), [])
        assert not any(len(l) for l in away.lists())
        got, rows, _ = call(renderer, Radiance(away), pattern, want_rows=True)
        assert (bits(got) == 0x7FC12345).all() and (bits(rows) == 0).all()
        assert renderer.grad_ordered_stats() == {"records": 0, "gaussians": 0, "longest": 0, "mismatches": 0}
        assert [len(a) for a in renderer.grad_records()] == [0, 0, 0]
        # a scene of no Gaussians
        renderer.set_gaussians(b.sc.g[:0])
        renderer.radiance_rays_grad_rays_device(b.nrays, b.t[0].data_ptr(), 0, b.t[1].data_ptr(), b.t[2].data_ptr(), table.data_ptr(), 0, 0)
        renderer.sync()
        assert (bits(table.cpu().numpy()) == 0x7FC12345).all()


def test_a_large_bundle_then_a_small_one(renderer, oracle):
    """The record buffers have grown for the aimed bundle; the small one behind it reads nothing of it"""
    big = bundle_of(renderer, oracle, "rad", "aimed 64x64")
    with ordered(renderer):
        call(renderer, big)
        assert renderer.grad_ordered_stats()["records"] == O.record_count(big.lens(1e-9, "vcl-as"), True)
    small = bundle_of(renderer, oracle, "rad", "small 5")
    bit_for_bit(renderer, small)
    tb = bundle_of(renderer, oracle, "T", "small 9 ns=5")
    bit_for_bit(renderer, tb)


def test_records_before_any_ordered_call_and_a_short_cap(pkg, oracle):
    sc = G.scene(oracle, "small 9")
    r = pkg.Renderer(0)
    try:
        assert [len(a) for a in r.grad_records()] == [0, 0, 0]
        assert r.grad_ordered_stats() == {"records": 0, "gaussians": 0, "longest": 0, "mismatches": 0}
        setup(r, sc.g)
        atomic = r.radiance_rays_grad(sc.o, sc.d, sc.gr)               # the default is off: the atomic path, no records
        assert [len(a) for a in r.grad_records()] == [0, 0, 0]
        r.set_grad_ordered(True)
        got = r.radiance_rays_grad(sc.o, sc.d, sc.gr)
        gauss, ray, rows = r.grad_records()
        m = len(gauss)
        assert m == sum(len(l) for l in sc.lists()) > 1
        val, Ssum = G.model(sc, "vcl-as")
        assert (np.abs(G.table_of(got) - G.table_of(atomic)) <= 2 * G.bound(Ssum)).all()
        n = C.c_size_t()
        u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        keep = (gauss.copy(), ray.copy(), rows.copy())
        rc = r._L.vrt_hip_get_grad_records(r._h, gauss.ctypes.data_as(u32p), ray.ctypes.data_as(u32p), rows.ctypes.data_as(f32p), m - 1, C.byref(n))
        assert rc == -1 and n.value == m                               # VRT_HIP_ERR_INVALID, the count reported, nothing copied
        assert all((a == k).all() for a, k in zip((gauss, ray, rows), keep))
    finally:
        r.close()


def test_environment_switch(pkg, oracle):
    sc = G.scene(oracle, "small 5")
    old = os.environ.get("VRT_HIP_GRAD_ORDERED")
    os.environ["VRT_HIP_GRAD_ORDERED"] = "1"
    try:
        r = pkg.Renderer(0)
    finally:
        if old is None:
            del os.environ["VRT_HIP_GRAD_ORDERED"]
        else:
            os.environ["VRT_HIP_GRAD_ORDERED"] = old
    try:
        setup(r, sc.g)
        r.radiance_rays_grad(sc.o, sc.d, sc.gr)
        assert r.grad_ordered_stats()["records"] == sum(len(l) for l in sc.lists())
    finally:
        r.close()


# ---- autograd: the renderer's switch decides ----
def test_autograd_backward_is_reproducible(renderer, oracle):
    import torch
    from sgrt_amd import autograd
    sc = G.scene(oracle, "grid16 scattered")
    renderer.set_options(*PAIRS["vcl-as"], 1e-9)
    t_o, t_d, t_g = cuda(sc.o), cuda(sc.d), cuda(sc.gr)
    s = cuda(np.linspace(0.2, 1.6, 5).astype(np.float32))
    t_w = cuda(np.random.default_rng(5).uniform(-1, 1, size=(len(sc.d), 5)).astype(np.float32))
    p = G.params64(sc.g)

    def grads(fn):
        ps = [torch.tensor(p[k], dtype=torch.float32, device="cuda", requires_grad=True) for k in ("mu", "albedo", "sigma", "magnitude")]
        if fn == "radiance":
            (autograd.radiance_rays(renderer, *ps, t_o, t_d) * t_g).sum().backward()
        else:
            (autograd.transmittance_bundle(renderer, *ps, t_o, t_d, s) * t_w).sum().backward()
        torch.cuda.synchronize()
        return [None if q.grad is None else q.grad.cpu().numpy() for q in ps]

    with ordered(renderer):
        for fn in ("radiance", "transmittance"):
            a, b = grads(fn), grads(fn)
            assert renderer.grad_ordered_stats()["records"] > 0           # backward took the ordered path
            seen = 0
            for x, y in zip(a, b):
                assert (x is None) == (y is None)
                if x is not None:
                    assert (bits(x) == bits(y)).all()
                    seen += int(np.abs(x).max() > 0)
            assert seen >= 3
