"""The scene set from device memory (vrt_hip_set_gaussians_device, csrc/vrt_scene_kernel.hip) on the GPU.  The yardstick is always the
same scene set through set_gaussians_soa(..., alpha=...) on a second renderer: frames, queries, bundles, the ray rows of the gradient
bundles, statistics and the Morton index must be the same bit for bit (the gradient TABLE is summed with float atomics and is held to
the float64 model of tests/grad_bundle_scenes.py instead).  Scenes: tests/scene_device_scenes.py, which tests/test_scene_device_scenes.py
holds to account on the CPU.
"""
import numpy as np
import pytest

import block_scenes as B
import grad_bundle_scenes as G
import scene_device_scenes as D
import trans_grad_bundle_scenes as TG

pytestmark = pytest.mark.gpu

FRAME = 64          # pixels per side of the tiled frame
TILE = 2.0 / 4      # 4 x 4 tiles


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b, what):
    """Equal bit for bit (a NaN equals the same NaN)."""
    assert np.shape(a) == np.shape(b), what
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=str(what))


def host_set(r, g):
    mu, alb, sig, mag = D.packed(g)
    r.set_gaussians_soa(mu, alb[:, :3], sig, mag, alpha=np.ascontiguousarray(alb[:, 3]))


def device_set(r, g, stream=None):
    """The scene from cuda tensors on torch's current stream (or `stream`).  Returns the tensors: the caller keeps them while it likes."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        t = [torch.from_numpy(a).cuda() for a in D.packed(g)]
        r.set_gaussians_device(len(g), *[x.data_ptr() for x in t], stream=s.cuda_stream)
    return t


@pytest.fixture(scope="module")
def host_r(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def dev_r(renderer, pkg, oracle):
    yield renderer
    renderer.enable_stats(False)
    renderer.set_ray_index(0)
    renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    renderer.clear_tiles()
    renderer.set_gaussians(oracle.grid_scene(2))      # a host update: forgets the torch streams the test enqueued on


def camera(oracle):
    if "cam" not in _shared:
        _shared["cam"] = B._camera(oracle, FRAME, FRAME)
    return _shared["cam"]


_shared = {}


def frame(r, oracle):
    """A tiled frame: (packed pixels, radiance)."""
    plane, view, origin = camera(oracle)
    r.set_plane(FRAME, FRAME, *plane)
    r.tile_gaussians(TILE, TILE, view)
    img, rad = r.render(origin)
    return img.copy(), rad.copy()


def everything(r, oracle):
    """What a scene gives through every path that reads it, by name."""
    o, d = D.rays()
    out = {}
    r.enable_stats(True)
    out["radiance"], out["pixels"] = r.radiance_rays(o, d, want_image=True)
    out["ray_stats"] = r.ray_stats()
    r.enable_stats(False)
    out["T"] = r.transmittance_bundle(o, d, D.SAMPLES)
    out["depth"] = r.depth_bundle(o, d, D.LEVELS)
    if r.n:
        _, rows = r.radiance_rays_grad(o, d, D.seeded_grad((len(d), 4), 31), want_table=False, want_rays=True)
        out["grad rows origin"], out["grad rows dir"] = rows["origin"], rows["dir"]
        _, gs, rows = r.transmittance_bundle_grad(o, d, D.SAMPLES, D.seeded_grad((len(d), len(D.SAMPLES)), 32), want_table=False, want_rays=True)
        out["tgrad samples"], out["tgrad rows origin"], out["tgrad rows dir"] = gs, rows["origin"], rows["dir"]
    out["query T"] = r.transmittance(o, d[0], D.SAMPLES)
    out["query radiance"] = r.radiance(np.tile(o, (8, 1)), d[:8])
    out["frame pixels"], out["frame radiance"] = frame(r, oracle)
    return out


def compare(a, b, what):
    assert a.keys() == b.keys()
    for k in b:
        if isinstance(b[k], dict):
            assert a[k] == b[k], (what, k, a[k], b[k])
        else:
            same(a[k], b[k], (what, k))


# ---- 1. the same bits as the host setter ----
@pytest.mark.parametrize("n", D.SIZES)
def test_same_bits_as_the_host_setter(dev_r, host_r, oracle, n):
    g = D.cloud(oracle, n)
    host_set(host_r, g)
    keep = device_set(dev_r, g)
    assert dev_r.n == host_r.n == n
    a, b = everything(dev_r, oracle), everything(host_r, oracle)
    print(n, b["ray_stats"], "peak", float(b["radiance"].max()), "frame peak", float(b["frame radiance"].max()))
    if n >= 63:
        assert b["radiance"].max() > 0 and b["frame radiance"].max() > 0       # not a comparison of darkness
    compare(a, b, n)
    del keep


def test_gradient_table_of_a_device_set_scene_against_the_model(dev_r, oracle):
    sc = G.scene(oracle, "small 9")
    dev_r.set_options(*G.PAIRS["vcl-as"], 1e-9)
    keep = device_set(dev_r, sc.g)
    got = G.table_of(dev_r.radiance_rays_grad(sc.o, sc.d, sc.gr))
    val, Ssum = G.model(sc, "vcl-as", 1e-9)
    assert np.isfinite(got).all() and np.abs(val).max() > 0
    excess = np.abs(got - val) - G.bound(Ssum)
    assert excess.max() <= 0, (np.unravel_index(np.argmax(excess), excess.shape), excess.max())
    del keep


# ---- 2. albedo_scale ----
def block_frame(pkg, r, sc, set_scene):
    """block_scenes' frame (tests/test_gpu_block.py: one tile, exact kernels, statistics on) of a scene set by set_scene."""
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, B.EPS_TEST)
    r.set_table_step(0.0)
    r.set_cull_prune(B.KAPPA)
    r.enable_stats(True)
    keep = set_scene(r, sc.g)
    r.set_plane(sc.w, sc.h, *sc.plane)
    r.tile_gaussians(sc.tw, sc.th, sc.view)
    img, rad = r.render(sc.origin)
    st = r.stats()
    del keep
    return img.copy(), rad.copy(), st


def restore(pkg, r):
    r.enable_stats(False)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    r.set_table_step(pkg.TABLE_STEP_DEFAULT)
    r.set_cull_prune(6.0)
    r.clear_tiles()


def factor_scene(oracle, kind):
    return D.all_nan_albedo(oracle) if kind == "albedo-nan" else B.scene(oracle, ("factors", kind))


@pytest.mark.parametrize("kind", ["albedo4", "albedo-inf", "albedo-nan"])
def test_albedo_scale_is_the_host_setters(pkg, dev_r, host_r, oracle, kind):
    sc = factor_scene(oracle, kind)
    dim = D.dimmed(sc)
    try:
        d1, h1 = block_frame(pkg, dev_r, sc, device_set), block_frame(pkg, host_r, sc, host_set)
        d2, h2 = block_frame(pkg, dev_r, dim, device_set), block_frame(pkg, host_r, dim, host_set)    # the pending value is resolved AGAIN
    finally:
        restore(pkg, dev_r)
        restore(pkg, host_r)
    for (di, dr, ds), (hi, hr, hs), what in ((d1, h1, kind), (d2, h2, kind + " dimmed")):
        print(what, {k: (ds[k], hs[k]) for k in ("lane_entries", "lane_pairs", "shaded_blocks")})
        same(di, hi, what)
        same(dr, hr, what)
        assert ds["lane_entries"] == hs["lane_entries"] and ds["lane_pairs"] == hs["lane_pairs"] and hs["lane_entries"] > 0, what
    if kind != "albedo-nan":
        assert h1[2]["lane_entries"] > h2[2]["lane_entries"]      # a quarter of the budget prunes less: the scale of 4 was in force


# ---- 3. the index on the device ----
@pytest.mark.parametrize("order", ["index on before the update", "index switched on after the update"])
@pytest.mark.parametrize("name", D.INDEX_NAMES)
def test_index_built_on_the_device(dev_r, host_r, oracle, name, order):
    g = D.index_scenes(oracle)[name]
    o, d = D.rays()
    want = D.morton_order(g)
    host_r.set_ray_index(1)
    host_set(host_r, g)
    host_r.enable_stats(True)
    dev_r.enable_stats(True)
    try:
        rad_h = host_r.radiance_rays(o, d)
        st_h, ist_h, perm_h = host_r.ray_stats(), host_r.ray_index_stats(), host_r.ray_index_perm()
        if order.startswith("index on"):
            dev_r.set_ray_index(1)
            keep = device_set(dev_r, g)
            same(dev_r.ray_index_perm(), want, (name, "the update builds the index"))
        else:
            dev_r.set_ray_index(0)
            keep = device_set(dev_r, g)
            dev_r.set_ray_index(1)
            with pytest.raises(Exception):
                dev_r.ray_index_perm()                             # the next bundle builds it
        rad_d = dev_r.radiance_rays(o, d)
        st_d, ist_d, perm_d = dev_r.ray_stats(), dev_r.ray_index_stats(), dev_r.ray_index_perm()
        dev_r.set_ray_index(0)
        rad_off = dev_r.radiance_rays(o, d)
        assert dev_r.ray_index_stats()["indexed"] == 0
    finally:
        host_r.enable_stats(False)
        host_r.set_ray_index(0)
    print(name, order, ist_h, st_h)
    same(perm_h, want, (name, "host perm is the model's"))
    same(perm_d, want, (name, "device perm"))
    assert ist_d == ist_h and ist_h["indexed"] == 1 and ist_h["leaves"] == -(-len(g) // D.LEAF), (name, ist_d, ist_h)
    assert st_d == st_h, (name, st_d, st_h)
    same(rad_d, rad_h, name)
    same(rad_d, rad_off, (name, "index on is index off"))
    del keep


# ---- 4. stream order, no synchronisation in between ----
@pytest.mark.parametrize("streams", ["one stream", "set on one stream, bundles on another"])
def test_stream_order_without_synchronisation(dev_r, host_r, oracle, streams):
    import torch
    scenes = {"A": D.cloud(oracle, 1000), "B": D.cloud(oracle, 130)}
    o, d = D.rays()
    want = {}
    for k, g in scenes.items():
        host_set(host_r, g)
        want[k] = host_r.radiance_rays(o, d)
    assert want["A"].max() > 0 and want["B"].max() > 0 and not np.array_equal(want["A"], want["B"])
    t_o, t_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    outs = [torch.full((len(d), 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
    dev = {k: [torch.from_numpy(a).cuda().reshape(-1) for a in D.packed(g)] for k, g in scenes.items()}
    src = [torch.zeros_like(t) for t in dev["A"]]                   # what the setter reads: room for the larger scene
    keep = device_set(dev_r, scenes["A"])                           # the renderer's buffers at the larger size: nothing grows below
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    s2 = s1 if streams == "one stream" else torch.cuda.Stream()

    def update(k):
        with torch.cuda.stream(s1):
            for dst, t in zip(src, dev[k]):
                dst[:t.numel()].copy_(t)
            dev_r.set_gaussians_device(len(scenes[k]), *[t.data_ptr() for t in src], stream=s1.cuda_stream)

    def bundle(i):
        dev_r.radiance_rays_device(len(d), t_o.data_ptr(), False, t_d.data_ptr(), d_radiance=outs[i].data_ptr(), stream=s2.cuda_stream)

    update("A")
    bundle(0)
    with torch.cuda.stream(s1):
        for t in src:
            t.fill_(0.37)                                           # the caller's arrays are its own again once the call returns
    bundle(1)                                                       # still scene A
    update("B")                                                     # another N within the reserved capacity
    bundle(2)
    update("A")
    bundle(3)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in outs]
    for i, k in enumerate("AABA"):
        same(got[i], want[k], (streams, i, k))
    del keep


# ---- 5. state transitions ----
def test_options_after_a_device_update_rebuild_from_the_columns(pkg, dev_r, host_r, oracle):
    g = D.cloud(oracle, 130)
    o, d = D.rays()
    out = []
    for r, set_scene in ((dev_r, device_set), (host_r, host_set)):
        r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        keep = set_scene(r, g)
        first = r.radiance_rays(o, d)
        r.set_options(pkg.EXP_LIBM, pkg.ERF_LIBM, 1e-4)            # another Exp kind and another cull_eps: the tables are rebuilt lazily
        out.append((first, r.radiance_rays(o, d), *frame(r, oracle)))
        r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        del keep
    for a, b, what in zip(out[0], out[1], ("before", "bundle after", "frame pixels after", "frame radiance after")):
        same(a, b, what)
    assert not np.array_equal(out[1][0], out[1][1])                 # the options changed something


def test_device_and_host_updates_alternate(dev_r, host_r, oracle):
    A, Bq = D.cloud(oracle, 130), D.cloud(oracle, 65)
    o, d = D.rays()
    want = {}
    for k, g in (("A", A), ("B", Bq)):
        host_set(host_r, g)
        want[k] = (host_r.radiance_rays(o, d), *frame(host_r, oracle))
    keep = device_set(dev_r, A)
    host_set(dev_r, Bq)                                             # device then host
    for a, b in zip((dev_r.radiance_rays(o, d), *frame(dev_r, oracle)), want["B"]):
        same(a, b, "device then host")
    keep = device_set(dev_r, A)                                     # host then device
    for a, b in zip((dev_r.radiance_rays(o, d), *frame(dev_r, oracle)), want["A"]):
        same(a, b, "host then device")
    del keep


def test_host_tile_lists_are_dropped_as_after_the_host_setter(pkg, dev_r, host_r, oracle):
    g, g2 = D.cloud(oracle, 130), D.cloud(oracle, 65)
    plane, view, origin = camera(oracle)
    tiles = {"tw": 2.0, "th": 2.0, "w": 1, "h": 1, "offsets": np.array([0, len(g)], np.uint32), "indices": np.arange(len(g), dtype=np.uint32)}
    out = []
    for r, set_scene in ((dev_r, device_set), (host_r, host_set)):
        host_set(r, g)
        r.set_plane(FRAME, FRAME, *plane)
        r.set_tiles(tiles)
        assert r.tile_counts().sum() == len(g)
        keep = set_scene(r, g2)                                     # the lists index another scene: untiled
        with pytest.raises(pkg.VrtHipError):
            r.tile_counts()
        img, rad = r.render(origin)
        out.append((img.copy(), rad.copy()))
        del keep
    same(out[0][0], out[1][0], "pixels")
    same(out[0][1], out[1][1], "radiance")
    assert out[1][1].max() > 0


def test_copy_state_takes_the_pending_albedo_scale_along(pkg, dev_r, host_r, oracle):
    sc = B.scene(oracle, ("factors", "albedo4"))
    L = pkg.lib()
    mirror = pkg.Renderer(0)
    try:
        dev_r.set_options(pkg.EXP_VCL, pkg.ERF_AS, B.EPS_TEST)
        dev_r.set_table_step(0.0)
        dev_r.set_cull_prune(B.KAPPA)
        keep = device_set(dev_r, sc.g)                              # no frame in between: the scale is still pending
        assert L.vrt_hip_copy_state(mirror._h, dev_r._h) == 0
        mirror.n = dev_r.n
        mirror.enable_stats(True)
        mirror.set_plane(sc.w, sc.h, *sc.plane)
        mirror.tile_gaussians(sc.tw, sc.th, sc.view)
        img, rad = mirror.render(sc.origin)
        st = mirror.stats()
        hi, hr, hs = block_frame(pkg, host_r, sc, host_set)
        del keep
    finally:
        mirror.close()
        restore(pkg, dev_r)
        restore(pkg, host_r)
    same(img, hi, "mirror pixels")
    same(rad, hr, "mirror radiance")
    assert st["lane_entries"] == hs["lane_entries"] and st["lane_pairs"] == hs["lane_pairs"] and hs["lane_entries"] > 0


def test_state_generation_advances_by_one(pkg, dev_r, oracle):
    L = pkg.lib()
    before = L.vrt_hip_state_generation(dev_r._h)
    keep = device_set(dev_r, D.cloud(oracle, 65))
    assert L.vrt_hip_state_generation(dev_r._h) == before + 1
    del keep


# ---- 6. refusals ----
def test_refusals_change_nothing(pkg, dev_r, oracle):
    L = pkg.lib()
    g = D.cloud(oracle, 130)
    o, d = D.rays()
    keep = device_set(dev_r, g)
    before = dev_r.radiance_rays(o, d)
    gen = L.vrt_hip_state_generation(dev_r._h)
    ptrs = [t.data_ptr() for t in keep]
    for k in range(4):
        with pytest.raises(pkg.VrtHipError, match="NULL"):
            dev_r.set_gaussians_device(5, *[0 if i == k else p for i, p in enumerate(ptrs)])
    with pytest.raises(pkg.VrtHipError, match="too many"):
        dev_r.set_gaussians_device(0xFFFFFFF1, *ptrs)
    assert dev_r.n == len(g) and L.vrt_hip_state_generation(dev_r._h) == gen
    same(dev_r.radiance_rays(o, d), before, "after the refusals")
    assert before.max() > 0
    dev_r.set_gaussians_device(0, 0, 0, 0, 0)                       # nothing, from nowhere: legal
    assert dev_r.n == 0 and L.vrt_hip_state_generation(dev_r._h) == gen + 1
    assert (dev_r.radiance_rays(o, d) == 0).all()
    del keep


# ---- 7. autograd ----
def parameters(g, device):
    import torch
    p = G.params64(g)
    return [torch.tensor(p[k], dtype=torch.float32, device=device, requires_grad=True) for k in ("mu", "albedo", "sigma", "magnitude")]


@pytest.mark.parametrize("what", ["radiance", "T", "depth"])
def test_autograd_cuda_parameters_against_cpu_parameters(dev_r, oracle, what):
    import torch
    from sgrt_amd import autograd
    dev_r.set_options(*G.PAIRS["vcl-as"], 1e-9)
    if what == "radiance":
        sc = G.scene(oracle, "small 9")
        weight, values = sc.gr, None
    else:
        case = TG.case(oracle, f"{what} small 9")
        sc, weight, values = case.sc, case.g, (case.s if what == "T" else case.tau)
    runs = {}
    for where in ("cuda", "cpu"):
        ps = parameters(sc.g, where)
        t_o = torch.tensor(sc.o, dtype=torch.float32, device="cuda", requires_grad=True)
        t_d = torch.tensor(sc.d, dtype=torch.float32, device="cuda", requires_grad=True)
        if what == "radiance":
            out = autograd.radiance_rays(dev_r, *ps, t_o, t_d)
        else:
            fn = autograd.transmittance_bundle if what == "T" else autograd.depth_bundle
            out = fn(dev_r, *ps, t_o, t_d, torch.tensor(values, dtype=torch.float32, device="cuda"))
        fwd = out.detach().cpu().numpy()
        live = np.isfinite(fwd)
        torch.where(torch.from_numpy(live).cuda(), out * torch.from_numpy(np.ascontiguousarray(weight, np.float32)).cuda(), torch.zeros_like(out)).sum().backward()
        assert all(p.grad is None or p.grad.device == p.device for p in ps)
        runs[where] = (fwd, t_o.grad.cpu().numpy(), t_d.grad.cpu().numpy(), [None if p.grad is None else p.grad.cpu().numpy() for p in ps], live)
    c, h = runs["cuda"], runs["cpu"]
    for a, b, name in zip(c[:3], h[:3], ("output", "origins.grad", "dirs.grad")):
        same(a, b, (what, name))
    assert np.abs(h[1]).max() > 0 and np.abs(h[2]).max() > 0
    mu, alb, sig, mag = c[3]
    hmu, halb, hsig, hmag = h[3]
    if what == "radiance":
        got = G.table_of({"albedo": alb, "mu": mu, "sigma": sig, "magnitude": mag})
        ref = G.table_of({"albedo": halb, "mu": hmu, "sigma": hsig, "magnitude": hmag})
        bound = G.bound(G.model(sc, "vcl-as")[1])
    else:
        assert alb is None and halb is None
        got = TG.table_of({"mu": mu, "sigma": sig, "magnitude": mag})
        ref = TG.table_of({"mu": hmu, "sigma": hsig, "magnitude": hmag})
        s = values if what == "T" else c[0]
        bound = TG.bound(TG.bundle_tgrad(case, "vcl-as", 1e-9, s=s, g=np.where(c[4], weight, 0.0).astype(np.float32)).S)
    assert np.abs(ref).max() > 0
    assert (np.abs(got - ref) <= 2 * bound).all()


def test_one_gradient_step_with_cuda_parameters_lowers_the_loss(dev_r, oracle):
    import torch
    from sgrt_amd import autograd
    from test_gpu_grad_bundles import descent_case
    sc, target, h = descent_case(oracle)
    dev_r.set_options(*G.PAIRS["vcl-as"], 1e-9)
    t_o, t_d, t_t = torch.from_numpy(sc.o).cuda(), torch.from_numpy(sc.d).cuda(), torch.tensor(target, dtype=torch.float32, device="cuda")
    ps = parameters(sc.g, "cuda")

    def loss_of(ps):
        return 0.5 * ((autograd.radiance_rays(dev_r, *ps, t_o, t_d) - t_t) ** 2).sum()
    l0 = loss_of(ps)
    l0.backward()
    g2 = sum(float((p.grad.double() ** 2).sum()) for p in ps)
    assert g2 > 0
    with torch.no_grad():
        stepped = [(p - h * p.grad).detach() for p in ps]
    l1 = loss_of(stepped)
    l0, l1 = l0.item(), l1.item()
    assert l0 - l1 >= 0.5 * h * g2, (l0, l1, h, g2)
