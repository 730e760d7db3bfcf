"""The ray-bundle family as a state machine on the GPU (tests/bundle_state_scenes.py has the model, the generator and the driver;
tests/test_bundle_state_scenes.py shows on the CPU what the committed sequences reach and that the driver reports leaked state): ONE
long-lived context goes through a seeded sequence of scene, bundle, option, switch and plan changes with a bundle call after each --
host form, device form, back to back, or left in flight across the next change -- and every reproducible word must be what a FRESH,
plainly configured context gives, which itself is held to the oracle where the scene is small.  One case per committed seed, in-process;
the last test drives the same comparison through the torch.autograd face, the way a fitting loop uses the library.
"""
import time

import numpy as np
import pytest

import bundle_state_scenes as BS

pytestmark = pytest.mark.gpu
_reference = []


def reference(oracle):
    """The float64 references, computed once and shared by the cases"""
    if not _reference:
        _reference.append(BS.Reference(oracle))
    return _reference[0]


@pytest.mark.parametrize("seed, nsteps", BS.CASES, ids=[f"seed{s}-{n}" for s, n in BS.CASES])
def test_one_context_through_a_sequence_gives_what_fresh_contexts_give(pkg, oracle, seed, nsteps):
    A = BS.Gpu(pkg, oracle)
    lines = []
    t0 = time.perf_counter()
    try:
        bad = BS.run(A, lambda: BS.Gpu(pkg, oracle), seed, nsteps, reference(oracle), out=lines.append)
    finally:
        print("\n".join(lines))
        print(f"seed {seed}, {nsteps} steps: {time.perf_counter() - t0:.2f} s; {sum('left in flight' in l for l in lines)} bundles left in flight, "
              f"{sum('still running' in l for l in lines)} of them still running when the next state change and bundle had been issued")
        A.close()
    assert bad == [], "\n".join(bad)


# ---- a fitting loop through torch.autograd ----
LOOP = (("cloud-65", False), ("cloud-300", True), ("cloud-65~", True), ("cloud-300~", False), ("cloud-65", True), ("cloud-300", False))


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_a_fitting_loop_through_autograd_gives_what_fresh_contexts_give(pkg, oracle):
    """forward, backward and jvp of autograd.radiance_rays, transmittance_bundle and depth_bundle on cuda parameters, on ONE context whose
    scene every forward replaces from device memory: scenes of 65 and 300 Gaussians in turn, with and without a plan (bound with
    keep_lists around every library call), index and sort switched from step to step, the tables ordered so that every .grad is
    reproducible.  Every output, .grad and tangent is bit for bit what a fresh plain context gives through the host forms."""
    import torch
    from sgrt_amd import autograd as AG
    b = BS.Bundle("cloud-300", 130, False, 7)
    o, d = BS.rays_of(oracle, b)
    x = BS.inputs(b, 0)
    tau = np.ascontiguousarray(np.broadcast_to(BS.LEVELS, (len(d), 3)))
    side = torch.cuda.Stream()
    A = pkg.Renderer(0)
    A.set_grad_ordered(1)
    bad = []
    try:
        for step, (name, planned) in enumerate(LOOP):
            g = BS.scene(oracle, name)
            tangent_mu = np.random.default_rng(100 + step).uniform(-0.05, 0.05, size=(len(g), 3)).astype(np.float32)
            # what a fresh, plain context gives
            B = pkg.Renderer(0)
            try:
                B.set_gaussians(g)
                B.set_grad_ordered(1)
                want = {"L": B.radiance_rays(o, d), "T": B.transmittance_bundle(o, d, x["s_ray"]), "z": B.depth_bundle(o, d, tau)}
                want["L table"], want["L rows"] = B.radiance_rays_grad(o, d, x["gr"], want_rays=True)
                want["T table"], want["T grad_s"], want["T rows"] = B.transmittance_bundle_grad(o, d, x["s_ray"], x["gT"], want_rays=True)
                want["z table"], want["z grad_tau"], want["z rows"] = B.transmittance_bundle_grad(o, d, want["z"], x["gT"][:, :3], wrt=pkg.TGRAD_DEPTH,
                                                                                                 s_per_ray=True, want_rays=True)
                want["L jvp"] = B.radiance_rays_tangent(o, d, tangent={"mu": tangent_mu})
                want["T jvp"] = B.transmittance_bundle_tangent(o, d, x["s_ray"], tangent={"mu": tangent_mu})
                want["z jvp"] = B.transmittance_bundle_tangent(o, d, want["z"], tangent={"mu": tangent_mu}, wrt=pkg.TGRAD_DEPTH, s_per_ray=True)
            finally:
                B.close()
            assert want["L"].max() > 0 and (want["T"] < 1).any() and np.isfinite(want["z"]).any()      # not a comparison of darkness
            # the long-lived context, through autograd
            A.set_ray_index(step % 2)
            A.set_ray_sort((step // 2) % 2)
            plan = None
            if planned:
                A.set_gaussians(g)
                plan = A.ray_plan(o, d)
            with torch.cuda.stream(side) if step % 2 else torch.cuda.stream(torch.cuda.current_stream()):
                t_o, t_gr, t_gT = (torch.from_numpy(a).cuda() for a in (o, x["gr"], x["gT"]))
                t_mu_dot = torch.from_numpy(tangent_mu).cuda()
                for kind in ("L", "T", "z"):
                    mu, alb, sig, mag = (torch.from_numpy(a).cuda().requires_grad_(True) for a in BS.packed(g))
                    t_d = torch.from_numpy(d).cuda().requires_grad_(True)
                    if kind == "L":
                        fn = lambda m: AG.radiance_rays(A, m, alb, sig, mag, t_o, t_d, plan=plan)                       # noqa: E731
                        v, weight = None, t_gr
                    else:
                        v = torch.from_numpy(x["s_ray"] if kind == "T" else tau).cuda().requires_grad_(True)
                        call = AG.transmittance_bundle if kind == "T" else AG.depth_bundle
                        fn = lambda m: call(A, m, alb, sig, mag, t_o, t_d, v, plan=plan)                                # noqa: E731
                        weight = t_gT if kind == "T" else t_gT[:, :3].contiguous()
                    out = fn(mu)
                    finite = torch.where(torch.isfinite(out), out, torch.zeros_like(out))       # a depth of +inf gets and gives no gradient
                    (finite * weight).sum().backward()
                    _, jvp = torch.func.jvp(fn, (mu,), (t_mu_dot,))
                    table, rows = want[kind + " table"], want[kind + " rows"]
                    got = {kind: out, kind + " jvp": jvp, kind + " mu.grad": mu.grad, kind + " sigma.grad": sig.grad, kind + " magnitude.grad": mag.grad,
                           kind + " dirs.grad": t_d.grad}
                    exp = {kind: want[kind], kind + " jvp": want[kind + " jvp"], kind + " mu.grad": table["mu"], kind + " sigma.grad": table["sigma"],
                           kind + " magnitude.grad": table["magnitude"], kind + " dirs.grad": rows["dir"]}
                    if kind == "L":
                        got["L albedo.grad"], exp["L albedo.grad"] = alb.grad, table["albedo"]
                    else:
                        assert alb.grad is None
                        got[kind + " values.grad"], exp[kind + " values.grad"] = v.grad, want["T grad_s" if kind == "T" else "z grad_tau"]
                    torch.cuda.synchronize()
                    for k in exp:
                        same = np.array_equal(bits(got[k]), bits(exp[k]))
                        print(f"step {step} {name} plan={int(planned)} index={step % 2} sort={(step // 2) % 2} {k}: {'ok' if same else 'MISMATCH'}")
                        if not same:
                            bad.append(f"step {step} {name}: {k}")
            torch.cuda.synchronize()
            if plan is not None:
                plan.close()
    finally:
        A.close()
    assert bad == []
