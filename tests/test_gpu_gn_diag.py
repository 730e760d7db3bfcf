"""Gauss-Newton diagonal bundles on the GPU (vrt_hip_radiance_rays_gn_diag*, csrc/vrt_ray_gn_diag_kernel.hip) against the float64 model of
tests/gn_diag_scenes.py, within its bound B per entry (tests/test_gn_diag_scenes.py holds model, bound and scenes to account on the
CPU), and against the library's own gradient bundles where no model is needed."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import gn_diag_scenes as D
import grad_bundle_scenes as G
import ray_plan_scenes as P
from gn_diag_scenes import PAIRS, RAY_LCAP, RAY_PL

pytestmark = pytest.mark.gpu

POISON_BITS = 0x0DABCDEF                                        # a finite float32 of 1.06e-30 with a mantissa nobody computes
POISON = float(np.array([POISON_BITS], np.uint32).view(np.float32)[0])
f32p = C.POINTER(C.c_float)


def setup(renderer, g, pair="vcl-as", eps=1e-9):
    renderer.set_options(*PAIRS[pair], eps)
    renderer.set_gaussians(g)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """Bit for bit; says where not"""
    a, b = np.asarray(a, np.float32).reshape(np.shape(b)), np.asarray(b, np.float32)
    ne = bits(a) != bits(b)
    if ne.any():
        j = tuple(np.argwhere(ne)[0])
        print(f"{int(ne.sum())} of {ne.size} words differ, first at {j}: {a[j]!r} against {b[j]!r}")
    return not ne.any()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def poisoned(n):
    return np.full((n, 12), POISON_BITS, np.uint32).view(np.float32)


@contextlib.contextmanager
def switches(renderer, ordered=False, index=False, sort=False):
    renderer.set_grad_ordered(ordered)
    renderer.set_ray_index(index)
    renderer.set_ray_sort(sort)
    try:
        yield renderer
    finally:
        renderer.set_grad_ordered(False)
        renderer.set_ray_index(False)
        renderer.set_ray_sort(False)


def device_call(renderer, sc, w, table0=None, rays=None, stream=None, per_ray=None):
    """The device form over the scene's rays (all, or the slice `rays`) added into a copy of table0 (a poisoned table without): [N, 12]"""
    import torch
    rays = slice(None) if rays is None else rays
    o = sc.o if sc.o.size == 3 else sc.o[rays]
    d = sc.d[rays]
    t_o, t_d = cuda(np.asarray(o, np.float32)), cuda(np.asarray(d, np.float32))
    t_w = None if w is None else cuda(np.asarray(w, np.float32)[rays])
    table = cuda(poisoned(len(sc.g)) if table0 is None else table0)
    torch.cuda.synchronize()
    per = int(sc.o.size != 3) if per_ray is None else per_ray
    if stream is None:
        renderer.radiance_rays_gn_diag_device(len(d), t_o.data_ptr(), per, t_d.data_ptr(), 0 if t_w is None else t_w.data_ptr(), table.data_ptr())
    else:
        with torch.cuda.stream(stream):
            renderer.radiance_rays_gn_diag_device(len(d), t_o.data_ptr(), per, t_d.data_ptr(), 0 if t_w is None else t_w.data_ptr(), table.data_ptr(),
                                                  stream=stream.cuda_stream)
        stream.synchronize()
    renderer.sync()
    return table.cpu().numpy()


def host_call(renderer, sc, w, rays=None):
    rays = slice(None) if rays is None else rays
    o = sc.o if sc.o.size == 3 else sc.o[rays]
    return renderer.radiance_rays_gn_diag(o, sc.d[rays], None if w is None else np.asarray(w, np.float32)[rays])


def within(got, want, B, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    excess = np.abs(got - want) - B
    j = np.unravel_index(np.argmax(excess), excess.shape)
    on = B > 0
    print(f"{what}: worst |device - model| / B = {float((np.abs(got - want)[on] / B[on]).max()) if on.any() else 0.0:.3f}")
    assert excess[j] <= 0, (what, j, got[j], want[j], B[j])


def check_added_into_poison(got, Dm, B, nj, what):
    """got [N, 12]: the device form's table over a poisoned one.  The poison is one addend more of every written cell's sum, 2^-24 of it
    per addition: the bound's own summation term with |POISON| among the addends."""
    kept = nj > 0
    assert (bits(got)[~kept] == POISON_BITS).all(), what         # rows no ray keeps: not written at all
    assert (bits(got)[:, 9:] == POISON_BITS).all(), what         # columns 9..11 of every row
    within(got[kept][:, :9], POISON + Dm[kept], B[kept] + ((nj[kept] + 8.0) * 2.0 ** -24 * POISON)[:, None], what)


# ---- parity with the model: every emitter-chunk residue, RAY_PL either side, the long kernel's rounds, RAY_LCAP and the workspace ----
@pytest.mark.parametrize("wkind", ["seeded", "null"])
@pytest.mark.parametrize("eps", G.EPS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("name", D.NAMES)
def test_parity(renderer, oracle, name, pair, eps, wkind):
    sc = D.scene(oracle, name)
    setup(renderer, sc.g, pair, eps)
    w = D.weights(sc, wkind)
    Dm, B, nj = D.model(sc, pair, eps, wkind)
    renderer.enable_stats(True)
    try:
        host = host_call(renderer, sc, w)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    assert host.shape == (len(sc.g), 12) and host.dtype == np.float32
    within(host[:, :9], Dm, B, (name, pair, eps, wkind, "host"))
    assert (host[:, 9:] == 0).all() and (host[nj == 0] == 0).all()
    assert (host[:, :9] >= 0).all()                               # non-negative weights: every addend is a square
    got = device_call(renderer, sc, w)
    check_added_into_poison(got, Dm, B, nj, (name, pair, eps, wkind, "device"))
    lens = [len(l) for l in sc.lists(eps, PAIRS[pair][0])]
    assert st["rays"] == len(lens) and st["long_rays"] == sum(n > RAY_PL for n in lens) and st["short_rays"] == sum(n <= RAY_PL for n in lens)
    assert st["scratch_rays"] == sum(n > RAY_LCAP for n in lens)
    if "small" in name and len(sc.g) >= 5:
        assert (host[1] == 0).all() and (bits(got)[1] == POISON_BITS).all()         # magnitude 0: no ray keeps it, it gets nothing
    from sgrt_amd import grad_columns
    split = grad_columns(host)                                   # the table splits as a gradient's does
    assert split["albedo"].shape == (len(sc.g), 4) and split["mu"].shape == (len(sc.g), 3) and split["sigma"].shape == (len(sc.g),)
    assert (split["magnitude"] == host[:, 8]).all()


def test_three_long_rays_in_the_workspace(renderer, oracle):
    """Three rays of RAY_LCAP + 76 entries each: three workgroups of the one-wave-per-ray kernel at once, every one with 76 positions of
    running sums in its own slot of the workspace in device memory (a slot stride, a position stride, a slot shared by two workgroups)"""
    sc = D.workspace_bundle(oracle)
    setup(renderer, sc.g)
    lens = [len(l) for l in sc.lists()]
    assert lens == [RAY_LCAP + D.WORKSPACE_EXTRA] * 3
    w = D.weights(sc, "seeded")
    per_ray = D.rows(sc, "vcl-as")
    Dm, B, nj = D.diag_of(sc, per_ray, w)
    renderer.enable_stats(True)
    try:
        host = host_call(renderer, sc, w)
        st = renderer.ray_stats()
    finally:
        renderer.enable_stats(False)
    assert st["long_rays"] == 3 and st["scratch_rays"] == 3
    within(host[:, :9], Dm, B, "three long rays, atomic")
    with switches(renderer, ordered=True):
        got = host_call(renderer, sc, w)
        rec = records_by_ray(renderer)
        alone = {}
        for r in range(3):                                                                  # each ray alone: one workgroup, one slot
            assert (host_call(renderer, sc, w, rays=slice(r, r + 1))[:, :9] > 0).any()
            alone.update({(r, j): v for (_, j), v in records_by_ray(renderer).items()})
    assert len(rec) == 3 * len(sc.g) and all((rec[k] == alone[k]).all() for k in rec)    # a ray's share does not depend on its company
    _, Bo, _ = D.diag_of(sc, per_ray, w, ordered=True)
    within(got[:, :9], Dm, Bo, "three long rays, ordered")


def test_weights_need_not_be_positive(renderer, oracle):
    """The sum is linear in the weights: D for weights of both signs, entries of both signs, within the bound (which goes by |w|)"""
    sc = D.scene(oracle, "small 9")
    setup(renderer, sc.g)
    w = D.weights(sc, "seeded") * np.where(np.arange(len(sc.d) * 4).reshape(-1, 4) % 3 == 0, -1.0, 1.0).astype(np.float32)
    Dm, B, nj = D.diag_of(sc, D.rows(sc, "vcl-as"), w)
    assert (Dm < 0).any() and (Dm > 0).any()
    within(host_call(renderer, sc, w)[:, :9], Dm, B, "signed weights")


# ---- bundle shape ----
def records_by_ray(renderer):
    gauss, ray, rows = renderer.grad_records()
    assert len(set(zip(ray.tolist(), gauss.tolist()))) == len(gauss)                # ONE record per (ray, kept Gaussian), long rays too
    return {(int(r), int(j)): bits(row).copy() for j, r, row in zip(gauss, ray, rows)}


@pytest.mark.parametrize("kind", ["coherent", "scattered"])
def test_bundle_sizes_give_the_same_segments_ray_for_ray(renderer, oracle, kind):
    sc = D.scene(oracle, f"grid16 {kind}")
    setup(renderer, sc.g)
    w = D.weights(sc, "seeded")
    lists = sc.lists()
    per_ray = D.rows(sc, "vcl-as")
    with switches(renderer, ordered=True):
        full = None
        for n in (130, 1, 63, 64, 65):
            table = device_call(renderer, sc, w, np.zeros((len(sc.g), 12), np.float32), rays=slice(0, n))
            rec = records_by_ray(renderer)
            assert len(rec) == sum(len(l) for l in lists[:n]) and renderer.grad_ordered_stats()["mismatches"] == 0
            if full is None:
                full = rec
                assert any(len(l) > RAY_PL for l in lists) == (kind == "scattered")
                # the segments are the rays' own shares of D
                for r in (0, 64, 129):
                    idx, v, S = per_ray[r]
                    share, Bshare, _ = D.diag_of(sc, per_ray, w, rays=[r])
                    got = np.stack([full[(r, int(j))].view(np.float32) for j in idx]).astype(np.float64)
                    assert (np.abs(got - share[idx]) <= Bshare[idx]).all(), r
            else:
                assert all((full[k] == v).all() for k, v in rec.items()), n
            Dn, Bn, _ = D.diag_of(sc, per_ray, w, rays=range(n), ordered=True)
            within(table[:, :9], Dn, Bn, (kind, n))


def test_nothing_kept_no_gaussians_one_origin(renderer, oracle):
    import torch
    sc = D.scene(oracle, "small 9")
    setup(renderer, sc.g)
    w = D.weights(sc, "seeded")
    # a ray that keeps nothing, alone and among the others (per-ray origins: it passes fifty units from the scene)
    far_o, far_d = np.array([[50.0, 0.0, 0.0]], np.float32), np.array([[0.0, 1.0, 0.0]], np.float32)
    for eps in G.EPS:
        assert not G.R.kept(far_o, far_d, sc.g, eps).any()
    assert (renderer.radiance_rays_gn_diag(far_o, far_d) == 0).all()
    each_o = np.tile(sc.o, (len(sc.d), 1))
    for ordered in (False, True):
        with switches(renderer, ordered=ordered):
            t_o, t_d = cuda(far_o), cuda(far_d)
            table = cuda(poisoned(len(sc.g)))
            torch.cuda.synchronize()
            renderer.radiance_rays_gn_diag_device(1, t_o.data_ptr(), 1, t_d.data_ptr(), 0, table.data_ptr())
            renderer.sync()
            assert (bits(table.cpu().numpy()) == POISON_BITS).all()
            mixed_o = np.concatenate([each_o[:2], far_o, each_o[2:]])
            mixed_d = np.concatenate([sc.d[:2], far_d, sc.d[2:]])
            wm = np.concatenate([w[:2], [[1, 2, 3, 4]], w[2:]]).astype(np.float32)
            got = renderer.radiance_rays_gn_diag(mixed_o, mixed_d, wm)
            want = renderer.radiance_rays_gn_diag(sc.o, sc.d, w)
            if ordered:
                assert (bits(got) == bits(want)).all()
            else:
                assert (np.abs(got[:, :9].astype(np.float64) - want[:, :9]) <= 2 * D.summation_term(sc, "vcl-as")).all()
    # one origin for the bundle is the same origin per ray, bit for bit (ordered: no arrival order)
    with switches(renderer, ordered=True):
        one = renderer.radiance_rays_gn_diag(sc.o, sc.d, w)
        each = renderer.radiance_rays_gn_diag(np.tile(sc.o, (len(sc.d), 1)), sc.d, w)
        assert (bits(one) == bits(each)).all() and (one != 0).any()
    # a scene of no Gaussians: OK, nothing launched, the table untouched
    renderer.set_gaussians(sc.g[:0])
    t_o, t_d = cuda(sc.o), cuda(sc.d)
    table = cuda(poisoned(4))
    torch.cuda.synchronize()
    renderer.radiance_rays_gn_diag_device(len(sc.d), t_o.data_ptr(), 0, t_d.data_ptr(), 0, table.data_ptr())
    renderer.sync()
    assert (bits(table.cpu().numpy()) == POISON_BITS).all()
    assert renderer.radiance_rays_gn_diag(sc.o, sc.d).shape == (0, 12)
    setup(renderer, sc.g)


# ---- cross-checks that use no model: the library's own gradient bundles ----
@pytest.mark.parametrize("name", ["small 9", f"stack {RAY_PL}|{RAY_PL + 1}"])
def test_one_ray_one_channel_is_the_gradient_table_squared(renderer, oracle, name):
    """One ray, weights e_c: D is the square of radiance_rays_grad's table for g = e_c.  Either side is within its own bound of the same
    row v: |D - T^2| <= B + 2 |T| b + b^2 with b = grad_bundle_scenes.bound of the table."""
    sc = D.scene(oracle, name)
    setup(renderer, sc.g)
    per_ray = D.rows(sc, "vcl-as")
    for r in range(min(2, len(sc.d))):
        idx, v, S = per_ray[r]
        o = sc.origin(r)
        for c in range(4):
            e = np.zeros((len(sc.d), 4), np.float32)
            e[r, c] = 1.0
            T = G.table_of(renderer.radiance_rays_grad(o, sc.d[r:r + 1], e[r:r + 1]))
            got = renderer.radiance_rays_gn_diag(o, sc.d[r:r + 1], e[r:r + 1])[:, :9].astype(np.float64)
            _, B, _ = D.diag_of(sc, per_ray, e, rays=[r])
            b = np.zeros_like(T)
            b[idx] = G.bound(S[c])
            assert (T != 0).any() and (np.abs(got - T * T) <= B + 2 * np.abs(T) * b + b * b).all(), (name, r, c)


@pytest.mark.parametrize("name", ["grid16 scattered", f"stack {RAY_PL + 1}|{RAY_PL + 2}"])
def test_ordered_diagonal_is_the_sum_of_squares_of_the_gradient_records(renderer, oracle, name):
    """Four ordered gradient calls with g = sqrt(w_c) e_c: their records, summed per (ray, Gaussian) (a long ray files two), squared and
    summed in float64, against the ordered D -- within B"""
    sc = D.scene(oracle, name)
    setup(renderer, sc.g)
    w = D.weights(sc, "seeded")
    N = len(sc.g)
    with switches(renderer, ordered=True):
        got = host_call(renderer, sc, w)[:, :9].astype(np.float64)
        want = np.zeros((N, 9))
        for c in range(4):
            g = np.zeros((len(sc.d), 4), np.float32)
            g[:, c] = np.sqrt(w[:, c].astype(np.float64)).astype(np.float32)
            renderer.radiance_rays_grad(sc.o, sc.d, g)
            gauss, ray, rows = renderer.grad_records()
            per = np.zeros((len(sc.d), N, 9))
            np.add.at(per, (ray, gauss), rows.astype(np.float64))
            want += (per * per).sum(0)
    _, B, _ = D.model(sc, "vcl-as", 1e-9, "seeded", ordered=True)
    assert (want > 0).any()
    within(got, want, B, (name, "records of four gradient calls"))


# ---- reproducibility and switches ----
def test_ordered_bits_and_atomic_agreement(renderer, oracle):
    sc = D.scene(oracle, "grid16 scattered")
    setup(renderer, sc.g)
    w = D.weights(sc, "seeded")
    zero = np.zeros((len(sc.g), 12), np.float32)
    ref = None
    for index in (False, True):
        for sort in (False, True):
            with switches(renderer, ordered=True, index=index, sort=sort):
                runs = [host_call(renderer, sc, w) for _ in range(3)] + [device_call(renderer, sc, w, zero)]
                plan = renderer.ray_plan(sc.o, sc.d)
                with renderer.using(plan):
                    runs += [host_call(renderer, sc, w), device_call(renderer, sc, w, zero)]
                plan.close()
            ref = runs[0] if ref is None else ref
            for k, t in enumerate(runs):
                assert (bits(t) == bits(ref)).all(), (index, sort, k)
    Dm, B, nj = D.model(sc, "vcl-as", 1e-9, "seeded", ordered=True)
    within(ref[:, :9], Dm, B, "ordered")
    # The atomic table sums the same per-ray shares in arrival order: depth n_j against ceil(n_j / 64) + 6, together below n_j + 8 for
    # the n_j <= 130 of this bundle -- the summation term of B
    assert nj.max() <= 130
    atomic = host_call(renderer, sc, w)
    assert (np.abs(atomic[:, :9].astype(np.float64) - ref[:, :9]) <= D.summation_term(sc, "vcl-as")).all()
    assert (atomic[:, 9:] == 0).all()


@pytest.mark.parametrize("name", ["grid16 scattered", f"wide {RAY_LCAP + 1}"])
def test_ray_stats_are_the_radiance_bundles(renderer, oracle, name):
    sc = D.scene(oracle, name)
    setup(renderer, sc.g)
    renderer.enable_stats(True)
    try:
        for index in (False, True):
            with switches(renderer, index=index):
                renderer.radiance_rays(sc.o, sc.d)
                want, want_index = renderer.ray_stats(), renderer.ray_index_stats()
                host_call(renderer, sc, None)
                assert renderer.ray_stats() == want and want["rays"] == len(sc.d), (name, index)
                assert renderer.ray_index_stats() == want_index and want_index["indexed"] == index, (name, index)
    finally:
        renderer.enable_stats(False)


# ---- plans ----
@pytest.mark.parametrize("name", [f"stack {RAY_PL}|{RAY_PL + 1}", f"wide {RAY_LCAP + 1}"])
def test_planned_is_unplanned_on_the_long_lists(renderer, oracle, name):
    sc = D.scene(oracle, name)
    setup(renderer, sc.g)
    w = D.weights(sc, "seeded")
    for index in (False, True):
        with switches(renderer, ordered=True, index=index):
            want = host_call(renderer, sc, w)
            plan = renderer.ray_plan(sc.o, sc.d)
            with renderer.using(plan):
                got = host_call(renderer, sc, w)
            plan.close()
            assert (bits(got) == bits(want)).all() and (want != 0).any(), (name, index)


def test_a_stale_plan_is_refused_and_kept_lists_give_the_plans_sum(renderer, oracle):
    import torch
    fz = P.frozen_pair(oracle)
    setup(renderer, fz.A)
    plan = renderer.ray_plan(fz.o, fz.d)
    renderer.set_gaussians(fz.B)
    sc = fz.scene("B", frozen=True)
    w = D.weights(sc, "seeded")
    # strict: refused with the table untouched
    t_o, t_d, table = cuda(fz.o), cuda(np.asarray(fz.d, np.float32)), cuda(poisoned(len(fz.B)))
    torch.cuda.synchronize()
    renderer.set_ray_plan(plan)
    try:
        rc = renderer._L.vrt_hip_radiance_rays_gn_diag_device(renderer._h, len(fz.d), t_o.data_ptr(), 0, t_d.data_ptr(), None, table.data_ptr(), None)
        assert rc == -1 and b"stale" in renderer._L.vrt_hip_last_error(renderer._h)
        renderer.sync()
        assert (bits(table.cpu().numpy()) == POISON_BITS).all()
    finally:
        renderer.set_ray_plan(None)
    # KEEP_LISTS: B's Gaussians under A's lists
    with renderer.using(plan, keep_lists=True):
        got = host_call(renderer, sc, w)
    own = host_call(renderer, sc, w)
    plan.close()
    Dm, B, nj = D.diag_of(sc, D.rows(sc, "vcl-as"), w)
    within(got[:, :9], Dm, B, "B under A's lists")
    assert (got[fz.enter] == 0).all() and (own[fz.enter, :9].max(1) > 0).all()          # nothing new is picked up; B's own cull picks it up
    assert (got[fz.stay, :9].max(1) > 0).all()


# ---- refusals ----
def test_refusals(renderer, oracle, pkg):
    import torch
    sc = D.scene(oracle, "small 5")
    t_o, t_d, t_w = cuda(sc.o), cuda(sc.d), cuda(D.weights(sc, "seeded"))
    table = cuda(poisoned(len(sc.g)))
    torch.cuda.synchronize()
    dev, host, h, n = renderer._L.vrt_hip_radiance_rays_gn_diag_device, renderer._L.vrt_hip_radiance_rays_gn_diag, renderer._h, len(sc.d)
    o, d, w = (np.ascontiguousarray(a, np.float32) for a in (sc.o, sc.d, D.weights(sc, "seeded")))
    out = np.full((len(sc.g), 12), -1.0, np.float32)
    op, dp, wp, outp = (a.ctypes.data_as(f32p) for a in (o, d, w, out))
    try:
        setup(renderer, sc.g)
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_SPLINE, 1e-9)                      # a pair with jumps
        assert dev(h, n, t_o.data_ptr(), 0, t_d.data_ptr(), t_w.data_ptr(), table.data_ptr(), None) == -1
        assert b"radiance_rays_gn_diag" in renderer._L.vrt_hip_last_error(h)
        assert host(h, n, op, 0, dp, wp, outp) == -1
        with pytest.raises(pkg.VrtHipError):
            renderer.radiance_rays_gn_diag(sc.o, sc.d)
        setup(renderer, sc.g)                                                          # a supported pair again
        for ordered in (False, True):
            with switches(renderer, ordered=ordered):
                assert dev(h, n, t_o.data_ptr(), 0, t_d.data_ptr(), t_w.data_ptr(), None, None) == -1
                assert b"NULL diagonal table" in renderer._L.vrt_hip_last_error(h)
                assert dev(h, n, None, 0, t_d.data_ptr(), t_w.data_ptr(), table.data_ptr(), None) == -1
                assert dev(h, n, t_o.data_ptr(), 0, None, t_w.data_ptr(), table.data_ptr(), None) == -1
                assert dev(h, 2 ** 32, t_o.data_ptr(), 0, t_d.data_ptr(), t_w.data_ptr(), table.data_ptr(), None) == -1
                assert dev(None, n, t_o.data_ptr(), 0, t_d.data_ptr(), t_w.data_ptr(), table.data_ptr(), None) == -1
                assert host(h, n, op, 0, dp, wp, None) == -1 and host(h, n, None, 0, dp, wp, outp) == -1 and host(h, n, op, 0, None, wp, outp) == -1
                assert dev(h, 0, None, 0, None, None, None, None) == 0 and host(h, 0, None, 0, None, None, None) == 0      # nothing to do
        renderer.sync()
        torch.cuda.synchronize()
        assert (bits(table.cpu().numpy()) == POISON_BITS).all() and (out == -1.0).all()   # nothing was enqueued
    finally:
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)


def test_a_caller_stream_and_two_calls_into_one_table(renderer, oracle):
    import torch
    sc = D.scene(oracle, "grid16 scattered")
    setup(renderer, sc.g)
    w = D.weights(sc, "seeded")
    Dm, B, nj = D.model(sc, "vcl-as")
    st = torch.cuda.Stream()
    once = device_call(renderer, sc, w, np.zeros((len(sc.g), 12), np.float32), stream=st)
    twice = device_call(renderer, sc, w, once, stream=st)
    within(once[:, :9], Dm, B, "caller's stream")
    # the second call's n_j additions run on partial sums of up to 2 D: a third summation term
    within(twice[:, :9], 2 * Dm, 2 * B + D.summation_term(sc, "vcl-as"), "two calls into one table")
    assert (twice[:, 9:] == 0).all()


# ---- torch ----
def tensors(g, device):
    import torch
    p = G.params64(g)
    return [torch.tensor(p[k], dtype=torch.float32, device=device) for k in ("mu", "albedo", "sigma", "magnitude")]


@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_torch_returns_the_renderers_numbers(renderer, oracle, device):
    import torch
    from sgrt_amd import autograd, grad_columns
    sc = D.scene(oracle, "grid16 scattered")
    setup(renderer, sc.g)
    w = D.weights(sc, "seeded")
    with switches(renderer, ordered=True):
        plan = renderer.ray_plan(sc.o, sc.d)
        ps = tensors(sc.g, device)
        t_o, t_d, t_w = cuda(sc.o), cuda(sc.d), cuda(w)
        for p in (None, plan):
            before = renderer._plan
            zero = np.zeros((len(sc.g), 12), np.float32)
            for wt, t_wt in ((w, t_w), (None, None)):
                got = autograd.radiance_rays_gn_diag(renderer, *ps, t_o, t_d, weights=t_wt, plan=p)
                assert renderer._plan == before
                # The Renderer's own calls on the scene torch set, the host form AT ONCE: torch's call was enqueued on torch's current
                # stream (the null stream) and nothing here has waited for it yet -- the host form has to, it shares the context's queue,
                # records and workspace with it.
                host = grad_columns(host_call(renderer, sc, wt))
                dev = grad_columns(device_call(renderer, sc, wt, zero))
                assert len(got) == 4
                for t, q, k in zip(got, ps, ("mu", "albedo", "sigma", "magnitude")):
                    assert t.shape == q.shape and t.device == q.device and t.dtype == q.dtype and not t.requires_grad
                    assert same_bits(host[k], dev[k]) and (dev[k] != 0).any(), (k, p is not None, wt is not None)
                    assert same_bits(t.cpu().numpy(), dev[k]), (k, p is not None, wt is not None)
        got = autograd.radiance_rays_gn_diag(renderer, *ps, t_o, t_d, weights=t_w)
        plan.close()
    Dm, B, _ = D.model(sc, "vcl-as", 1e-9, "seeded", ordered=True)
    within(G.table_of({k: t.cpu().numpy() for k, t in zip(("mu", "albedo", "sigma", "magnitude"), got)}), Dm, B, ("torch", device))
