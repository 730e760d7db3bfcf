"""torch.autograd face of the ray bundles: radiance, transmittance and depth of caller-given rays as differentiable functions of the
Gaussians and of the rays.

    L = radiance_rays(renderer, mu, albedo, sigma, magnitude, origins, dirs)      # [nrays, 4], on cuda
    loss(L).backward()                                                            # mu.grad, albedo.grad, sigma.grad, magnitude.grad
    T = transmittance_bundle(renderer, mu, albedo, sigma, magnitude, origins, dirs, s)      # [nrays, ns]: masks, shadow rays
    z = depth_bundle(renderer, mu, albedo, sigma, magnitude, origins, dirs, tau)            # [nrays, nt]: depth maps, first hits

Forward is Renderer.radiance_rays_device, backward Renderer.radiance_rays_grad_rays_device (include/vrt_hip.h, "gradient bundles" and
"ray gradients"): the derivative with each ray's kept list held fixed, under {vcl_exp, expf} x {A&S erf, erff} only; the Gaussians'
gradients are summed with float atomics (not bitwise reproducible) -- unless the renderer's switch is on (Renderer.set_grad_ordered:
nothing changes here, backward calls the same entry points): then they are summed in a documented order, two backward passes give
bit-equal .grad, and every backward that asks for a table waits once for its stream.  transmittance_bundle and depth_bundle run
Renderer.transmittance_bundle_device / depth_bundle_device forward and Renderer.transmittance_bundle_grad_rays_device backward
("transmittance gradient bundles"), under the same rules; they are differentiable in s and tau as well, never in albedo (T does not depend on it).  The depth's derivative is that of the
ideal crossing T(depth) = tau; a depth of +inf, 0 or NaN gets no gradient.

Rays.  origins and dirs that require grad get one: origins [nrays, 3] d(loss) / d(origin) per ray, origins [3] its sum over the rays,
dirs the TANGENTIAL derivative (perpendicular to each direction: dirs are unit vectors, and the chain rule through
torch.nn.functional.normalize of a raw vector needs no more).  These rows come without atomic adds and are bitwise reproducible.
ctx.needs_input_grad decides what backward asks of the library: with no Gaussian parameter requiring grad no table is passed (a
pose-only fit pays for no atomic add), with no ray requiring grad the call is the one without ray rows.

Forward mode.  radiance_rays also works under torch.autograd.forward_ad and torch.func.jvp: its jvp is
Renderer.radiance_rays_tangent_device (include/vrt_hip.h, "tangent bundles"), J . v under the same fixed kept lists and the same pairs,
one pass, stored without atomic adds and bitwise reproducible.  The tangent table is built from the tangents of mu, albedo, sigma and
magnitude, the ray rows from those of origins ([3]: the same row for every ray) and dirs (only the part perpendicular to each direction
counts); a group without any tangent is not passed, and with no tangent at all nothing is issued.  transmittance_bundle and depth_bundle
work the same way: their jvp is Renderer.transmittance_bundle_tangent_device ("transmittance tangent bundles"), in T mode at the samples of
the forward, in depth mode at the depths it returned (a depth of +inf, 0 or NaN moves by exactly 0); the tangent of s or tau is a third
group, shaped and broadcast as s or tau is; albedo's tangent moves nothing.

A Gaussian whose magnitude is exactly 0 is dropped by every ray's cull and therefore receives NO gradient, magnitude.grad included
(although the true derivative is not 0): initialise magnitudes away from 0.

The scene.  Every forward REPLACES the renderer's scene by the parameters.  With all four parameter tensors on the renderer's cuda device
it does so on the device (Renderer.set_gaussians_device): the tensors are converted with .to(float32).contiguous() there and the scene
tables -- and the Morton index, when it is on -- are rebuilt by kernels on torch's current stream, with nothing copied to the host and
nothing waited for (but where a buffer of the renderer has to grow: a larger scene, the first call).  A fitting loop of bundles with
cuda parameters never blocks the host.  With any parameter tensor elsewhere (the CPU, another device) the scene goes through the host
as before: the four tensors are copied to the CPU and set_gaussians_soa waits for the device and rebuilds the tables.  Both ways make
the same scene, bit for bit.

Ray plans.  radiance_rays, transmittance_bundle and depth_bundle take plan=None: a RayPlan of the same rays (Renderer.ray_plan /
ray_plan_device; include/vrt_hip.h, "Ray plans").  With one, forward, backward and the jvp bind it around their library call with
keep_lists=True -- every forward sets the scene again, which a strict plan would refuse -- and put the renderer's previous binding back
afterwards: no call culls, all of them sum over the plan's lists, and the values are those of the function whose derivative backward and
jvp return.  Binding waits for bundles in flight; the default, plan=None, binds nothing and waits for nothing.
"""
import contextlib

import numpy as np
import torch

from . import GRAD_STRIDE, RAY_GRAD_STRIDE, TGRAD_DEPTH, TGRAD_T, grad_columns, ray_grad_columns


def _set_scene(renderer, mu, albedo, sigma, magnitude):
    """The scene of `renderer` replaced by the parameters: on the device when all four are on the renderer's cuda device, through the
    host otherwise (the module's docstring)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    params = (mu, albedo, sigma, magnitude)
    if getattr(renderer, "device", None) == dev.index and all(t.device == dev for t in params):
        # (the converted tensors may be temporaries: torch hands their memory on in stream order, behind the kernels that read them)
        m, a, s, g = (t.detach().to(torch.float32).contiguous() for t in params)
        n = s.numel()
        assert m.numel() == 3 * n and a.numel() == 4 * n and g.numel() == n
        renderer.set_gaussians_device(n, m.data_ptr(), a.data_ptr(), s.data_ptr(), g.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    else:
        host = [t.detach().to("cpu", torch.float32).contiguous().numpy() for t in params]
        renderer.set_gaussians_soa(host[0], host[1][:, :3], host[2], host[3], alpha=np.ascontiguousarray(host[1][:, 3]))


@contextlib.contextmanager
def _planned(renderer, plan):
    """The plan bound with its lists kept for one library call, the renderer's previous binding back behind it; nothing at all without a plan"""
    if plan is None:
        yield
    else:
        with renderer.using(plan, keep_lists=True):
            yield


def _rays(origins, dirs):
    """The rays as the library takes them, on torch's current device: (device, origins, dirs [nrays, 3], origin per ray).  Rays that are
    float32, contiguous and on that device already are taken as they are, not copied."""
    dev = torch.device("cuda", torch.cuda.current_device())
    o = origins.detach().to(dev, torch.float32).contiguous()
    d = dirs.detach().to(dev, torch.float32).contiguous().reshape(-1, 3)
    return dev, o, d, o.numel() != 3


def _remember(ctx, renderer, mu, albedo, sigma, magnitude, origins, dirs):
    """In ctx what backward (and jvp) need of the call: the renderer, the rays (_rays), the scene's size, and where and of what type the
    inputs are.  Returns what _rays returns."""
    dev, o, d, per_ray = _rays(origins, dirs)
    ctx.renderer, ctx.rays, ctx.n = renderer, (o, d, per_ray), sigma.numel()
    ctx.ray_like = (origins, dirs)
    ctx.devices = [t.device for t in (mu, albedo, sigma, magnitude)]
    ctx.dtypes = [t.dtype for t in (mu, albedo, sigma, magnitude)]
    return dev, o, d, per_ray


def _parameter_grads(ctx, table):
    """The table's columns as the gradients of (mu, albedo, sigma, magnitude), each on its parameter's device and in its type; None
    each where no table was asked for."""
    if table is None:
        return [None] * 4
    cols = grad_columns(table)
    return [cols[k].to(dev, dt) for k, dev, dt in zip(("mu", "albedo", "sigma", "magnitude"), ctx.devices, ctx.dtypes)]


def _outputs(ctx, first_param):
    """What a backward asks of the library, by ctx.needs_input_grad (the four parameters from index first_param, then origins, dirs):
    the cleared table or None, the ray rows or None."""
    o = ctx.rays[0]
    need = ctx.needs_input_grad
    table = torch.zeros((ctx.n, GRAD_STRIDE), dtype=torch.float32, device=o.device) if any(need[first_param:first_param + 4]) else None
    rows = (torch.zeros((ctx.rays[1].shape[0], RAY_GRAD_STRIDE), dtype=torch.float32, device=o.device)
            if any(need[first_param + 4:first_param + 6]) else None)
    return table, rows


def _ray_grads(ctx, rows):
    """The ray rows as the gradients of (origins, dirs) in their shapes, devices and types: one origin for the bundle gets the sum."""
    if rows is None:
        return [None, None]
    cols = ray_grad_columns(rows)
    origins, dirs = ctx.ray_like
    go = cols["origin"] if ctx.rays[2] else cols["origin"].sum(0)
    return [go.reshape(origins.shape).to(origins.device, origins.dtype), cols["dir"].reshape(dirs.shape).to(dirs.device, dirs.dtype)]


def _ptr(t):
    return t.data_ptr() if t is not None else 0


class _TangentBundle(torch.autograd.Function):
    """The library call of _RadianceRays.jvp as a Function of its own: under torch.func's transforms the tensors a jvp sees are wrapped,
    and a Function's forward is where torch hands over plain ones, whose memory can be named.  Not differentiable itself."""

    @staticmethod
    def forward(renderer, o, d, per_ray, table, rows, plan):
        out = torch.zeros((d.shape[0], 4), dtype=torch.float32, device=o.device)
        with _planned(renderer, plan):
            renderer.radiance_rays_tangent_device(d.shape[0], o.data_ptr(), per_ray, d.data_ptr(), d_tangent=_ptr(table), d_ray_tangent=_ptr(rows),
                                                  d_out=out.data_ptr(), stream=torch.cuda.current_stream(o.device).cuda_stream)
        return out

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass


class _RadianceRays(torch.autograd.Function):
    """forward and setup_context apart, as torch.func's transforms (jvp among them) ask of a Function: forward sets the scene and shades,
    setup_context remembers (from the inputs alone, which is all torch gives it: rays that forward had to convert are converted again)"""

    @staticmethod
    def forward(renderer, mu, albedo, sigma, magnitude, origins, dirs, plan):
        _set_scene(renderer, mu, albedo, sigma, magnitude)
        dev, o, d, per_ray = _rays(origins, dirs)
        out = torch.empty((d.shape[0], 4), dtype=torch.float32, device=dev)
        if d.shape[0]:
            with _planned(renderer, plan):
                renderer.radiance_rays_device(d.shape[0], o.data_ptr(), per_ray, d.data_ptr(), d_radiance=out.data_ptr(),
                                              stream=torch.cuda.current_stream(dev).cuda_stream)
        return out

    @staticmethod
    def setup_context(ctx, inputs, output):
        _remember(ctx, *inputs[:7])
        ctx.plan = inputs[7]
        # jvp sees None for an input without a tangent, not zeros, and passes no table for them.  The switch holds for backward too: it
        # sees None where the output's gradient is undefined, and then returns no gradients instead of those of a zero grad_out.
        ctx.set_materialize_grads(False)

    @staticmethod
    def jvp(ctx, _, t_mu, t_albedo, t_sigma, t_magnitude, t_origins, t_dirs, _p):
        """Forward mode (torch.autograd.forward_ad, torch.func.jvp): Renderer.radiance_rays_tangent_device over the scene and the rays
        of the forward, on torch's current stream.  The tangent table is built from the tangents of the four parameters, the ray rows
        from those of origins (one origin for the bundle: the same row for every ray) and dirs; a group none of whose inputs has a
        tangent is not passed at all, and with no tangent anywhere nothing is issued."""
        o, d, per_ray = ctx.rays
        nrays, n = d.shape[0], ctx.n

        def cols(shapes, tangents):
            return [torch.zeros(shape, dtype=torch.float32, device=o.device) if t is None else t.detach().to(o.device, torch.float32).reshape(shape)
                    for shape, t in zip(shapes, tangents)]
        table = rows = None
        if any(t is not None for t in (t_mu, t_albedo, t_sigma, t_magnitude)):          # grad_columns' layout
            table = torch.cat(cols(((n, 4), (n, 3), (n, 1), (n, 1), (n, GRAD_STRIDE - 9)), (t_albedo, t_mu, t_sigma, t_magnitude, None)), 1)
        if t_origins is not None or t_dirs is not None:                                 # ray_grad_columns' layout
            t_o = None if t_origins is None else t_origins.detach().reshape(-1, 3).expand(nrays, 3)      # [1, 3]: the same row for every ray
            rows = torch.cat(cols(((nrays, 3), (nrays, 1), (nrays, 3), (nrays, 1)), (t_o, None, t_dirs, None)), 1)
        if not (nrays and n) or (table is None and rows is None):
            return torch.zeros((nrays, 4), dtype=torch.float32, device=o.device)
        return _TangentBundle.apply(ctx.renderer, o, d, per_ray, table, rows, ctx.plan)

    @staticmethod
    def backward(ctx, grad_out):
        if grad_out is None:                 # (set_materialize_grads above) nothing flows back through the radiance
            return (None,) * 8
        o, d, per_ray = ctx.rays
        g = grad_out.to(o.device, torch.float32).contiguous()
        table, rows = _outputs(ctx, 1)
        if d.shape[0] and ctx.n and (table is not None or rows is not None):
            with _planned(ctx.renderer, ctx.plan):
                ctx.renderer.radiance_rays_grad_rays_device(d.shape[0], o.data_ptr(), per_ray, d.data_ptr(), g.data_ptr(), d_grad=_ptr(table),
                                                            d_grad_rays=_ptr(rows), stream=torch.cuda.current_stream(o.device).cuda_stream)
        return (None, *_parameter_grads(ctx, table), *_ray_grads(ctx, rows), None)


def radiance_rays(renderer, mu, albedo, sigma, magnitude, origins, dirs, plan=None):
    """Radiance [nrays, 4] (a cuda tensor on torch's current device and stream) of the rays through the scene of the four parameter
    tensors mu [N, 3], albedo [N, 4], sigma [N], magnitude [N], differentiable in those four and in the rays.  origins: [3] or
    [nrays, 3]; dirs: [nrays, 3], unit length (its gradient is the tangential one: see the module's docstring).  The scene of `renderer` is REPLACED by the parameters (see the module's docstring);
    backward must run before the renderer's scene or options change again.  Forward mode too: the module's docstring.  plan: a RayPlan of
    these rays, or None (the module's docstring, "Ray plans")."""
    return _RadianceRays.apply(renderer, mu, albedo, sigma, magnitude, origins, dirs, plan)


class _ProfileTangentBundle(torch.autograd.Function):
    """The library call of _Profile.jvp as a Function of its own, for the reason _TangentBundle gives.  Not differentiable itself."""

    @staticmethod
    def forward(renderer, wrt, o, d, per_ray, s, s_per_ray, table, rows, s_tangent, s_tangent_per_ray, plan):
        nrays, n = d.shape[0], s.shape[-1] if s.dim() else 1
        out = torch.zeros((nrays, n), dtype=torch.float32, device=o.device)
        with _planned(renderer, plan):
            renderer.transmittance_bundle_tangent_device(nrays, o.data_ptr(), per_ray, d.data_ptr(), s.data_ptr(), n, s_per_ray, wrt,
                                                         d_tangent=_ptr(table), d_ray_tangent=_ptr(rows), d_s_tangent=_ptr(s_tangent),
                                                         s_tangent_per_ray=s_tangent_per_ray, d_out=out.data_ptr(),
                                                         stream=torch.cuda.current_stream(o.device).cuda_stream)
        return out

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass


def _values(values):
    """A profile's samples or levels as the library takes them, on torch's current device: (values, per ray?, values per ray)"""
    v = values.detach().to(torch.device("cuda", torch.cuda.current_device()), torch.float32).contiguous()
    return v, v.dim() == 2, v.shape[-1] if v.dim() else 1


class _Profile(torch.autograd.Function):
    """transmittance_bundle (wrt = TGRAD_T: values = sample distances) and depth_bundle (TGRAD_DEPTH: values = levels).  forward and
    setup_context apart, as _RadianceRays and for its reason."""

    @staticmethod
    def forward(renderer, wrt, mu, albedo, sigma, magnitude, origins, dirs, values, plan):
        _set_scene(renderer, mu, albedo, sigma, magnitude)
        dev, o, d, per_ray = _rays(origins, dirs)
        nrays = d.shape[0]
        v, v_per_ray, n = _values(values)
        out = torch.empty((nrays, n), dtype=torch.float32, device=dev)
        if nrays and n:
            call = renderer.transmittance_bundle_device if wrt == TGRAD_T else renderer.depth_bundle_device
            with _planned(renderer, plan):
                call(nrays, o.data_ptr(), per_ray, d.data_ptr(), v.data_ptr(), n, v_per_ray, out.data_ptr(),
                     stream=torch.cuda.current_stream(dev).cuda_stream)
        return out

    @staticmethod
    def setup_context(ctx, inputs, output):
        renderer, wrt, mu, albedo, sigma, magnitude, origins, dirs, values, plan = inputs
        _remember(ctx, renderer, mu, albedo, sigma, magnitude, origins, dirs)
        ctx.plan = plan
        v, v_per_ray, _ = _values(values)
        ctx.wrt, ctx.values, ctx.v_per_ray, ctx.v_like = wrt, v, v_per_ray, values
        ctx.save_for_backward(output)
        ctx.save_for_forward(output)         # depth mode differentiates at the depths the forward returned, in either mode of AD
        ctx.set_materialize_grads(False)     # jvp sees None for an input without a tangent (_RadianceRays.setup_context)

    @staticmethod
    def jvp(ctx, _r, _w, t_mu, t_albedo, t_sigma, t_magnitude, t_origins, t_dirs, t_values, _p):
        """Forward mode: Renderer.transmittance_bundle_tangent_device over the scene and the rays of the forward, on torch's current
        stream -- T mode at the samples the forward took, depth mode at the depths it returned.  The tangent table is built from the
        tangents of mu, sigma and magnitude (albedo's moves nothing), the ray rows from those of origins and dirs as in
        _RadianceRays.jvp, the sample tangents from that of values, which broadcasts as values does; a group without a tangent is not
        passed, and with no tangent anywhere nothing is issued."""
        o, d, per_ray = ctx.rays
        (out,) = ctx.saved_tensors
        nrays, n = d.shape[0], ctx.n
        nv = out.shape[1]

        def cols(shapes, tangents):
            return [torch.zeros(shape, dtype=torch.float32, device=o.device) if t is None else t.detach().to(o.device, torch.float32).reshape(shape)
                    for shape, t in zip(shapes, tangents)]
        table = rows = st = None
        if any(t is not None for t in (t_mu, t_sigma, t_magnitude)):                    # grad_columns' layout
            table = torch.cat(cols(((n, 4), (n, 3), (n, 1), (n, 1), (n, GRAD_STRIDE - 9)), (None, t_mu, t_sigma, t_magnitude, None)), 1)
        if t_origins is not None or t_dirs is not None:                                 # ray_grad_columns' layout
            t_o = None if t_origins is None else t_origins.detach().reshape(-1, 3).expand(nrays, 3)
            rows = torch.cat(cols(((nrays, 3), (nrays, 1), (nrays, 3), (nrays, 1)), (t_o, None, t_dirs, None)), 1)
        if t_values is not None:
            st = t_values.detach().to(o.device, torch.float32).reshape(ctx.values.shape).contiguous()
        if not (nrays and n and nv) or (table is None and rows is None and st is None):
            return torch.zeros((nrays, nv), dtype=torch.float32, device=o.device)
        s, s_per_ray = (ctx.values, ctx.v_per_ray) if ctx.wrt == TGRAD_T else (out.detach(), True)
        return _ProfileTangentBundle.apply(ctx.renderer, ctx.wrt, o, d, per_ray, s, s_per_ray, table, rows, st, ctx.v_per_ray, ctx.plan)

    @staticmethod
    def backward(ctx, grad_out):
        if grad_out is None:                 # (set_materialize_grads above) nothing flows back through the profile
            return (None,) * 10
        o, d, per_ray = ctx.rays
        (out,) = ctx.saved_tensors
        nrays, n = out.shape
        g = grad_out.to(o.device, torch.float32).contiguous()
        table, rows = _outputs(ctx, 2)
        gv = torch.zeros((nrays, n), dtype=torch.float32, device=o.device)
        if nrays and n and ctx.n:
            # T mode: at the samples the forward took; depth mode: at the depths the forward returned, one row per ray
            s, s_per_ray = (ctx.values, ctx.v_per_ray) if ctx.wrt == TGRAD_T else (out, True)
            with _planned(ctx.renderer, ctx.plan):
                ctx.renderer.transmittance_bundle_grad_rays_device(nrays, o.data_ptr(), per_ray, d.data_ptr(), s.data_ptr(), n, s_per_ray, g.data_ptr(),
                                                                   ctx.wrt, d_grad=_ptr(table), d_grad_s=gv.data_ptr(), d_grad_rays=_ptr(rows),
                                                                   stream=torch.cuda.current_stream(o.device).cuda_stream)
        if not ctx.v_per_ray:                       # values shared by the rays: their gradient is the sum over the rays
            gv = gv.sum(0).reshape(ctx.values.shape)
        grads = _parameter_grads(ctx, table)
        grads[1] = None                             # albedo
        return (None, None, *grads, *_ray_grads(ctx, rows), gv.to(ctx.v_like.device, ctx.v_like.dtype), None)


def transmittance_bundle(renderer, mu, albedo, sigma, magnitude, origins, dirs, s, plan=None):
    """Transmittance [nrays, ns] (a cuda tensor on torch's current device and stream) at the sample distances s ([ns], shared by the
    rays, or [nrays, ns]) along the rays through the scene of the four parameter tensors, differentiable in mu, sigma, magnitude and
    s; albedo gets no gradient (None).  Forward mode too (forward_ad, torch.func.jvp): the module's docstring.  Rays, the replaced scene
    and the order of backward: as radiance_rays; so is plan."""
    return _Profile.apply(renderer, TGRAD_T, mu, albedo, sigma, magnitude, origins, dirs, s, plan)


def depth_bundle(renderer, mu, albedo, sigma, magnitude, origins, dirs, tau, plan=None):
    """The distance [nrays, nt] along each ray at which its transmittance falls to the levels tau ([nt], shared by the rays, or
    [nrays, nt]), differentiable in mu, sigma, magnitude and tau (the derivative of the ideal crossing; a result of +inf, 0 or NaN
    gets and gives no gradient); albedo gets no gradient (None).  Forward mode too: the module's docstring.  Rays, the replaced scene and
    the order of backward: as radiance_rays; so is plan."""
    return _Profile.apply(renderer, TGRAD_DEPTH, mu, albedo, sigma, magnitude, origins, dirs, tau, plan)


def radiance_rays_gn_diag(renderer, mu, albedo, sigma, magnitude, origins, dirs, weights=None, plan=None):
    """The diagonal of the Gauss-Newton matrix J^T W J of radiance_rays for the same arguments (Renderer.radiance_rays_gn_diag_device;
    include/vrt_hip.h, "Gauss-Newton diagonal bundles"): per parameter the sum over rays and channels of weights[r, c] ([nrays, 4], or
    None: all 1) times the squared derivative of channel c of ray r -- the Jacobi preconditioner of a CG solve on J and J^T, Marquardt's
    damping.  The scene of `renderer` is REPLACED by the parameters as radiance_rays does it; a plan is bound with keep_lists=True.
    Returns four tensors (mu, albedo, sigma, magnitude) shaped, placed and typed like the parameters, without graph."""
    with torch.no_grad():
        _set_scene(renderer, mu, albedo, sigma, magnitude)
        dev, o, d, per_ray = _rays(origins, dirs)
        n = sigma.numel()
        table = torch.zeros((n, GRAD_STRIDE), dtype=torch.float32, device=dev)
        w = None if weights is None else weights.detach().to(dev, torch.float32).contiguous().reshape(-1, 4)
        assert w is None or w.shape[0] == d.shape[0]
        if d.shape[0] and n:
            with _planned(renderer, plan):
                renderer.radiance_rays_gn_diag_device(d.shape[0], o.data_ptr(), per_ray, d.data_ptr(), d_weights=_ptr(w), d_diag=table.data_ptr(),
                                                      stream=torch.cuda.current_stream(dev).cuda_stream)
        cols = grad_columns(table)
        return tuple(cols[k].reshape(t.shape).to(t.device, t.dtype) for k, t in zip(("mu", "albedo", "sigma", "magnitude"), (mu, albedo, sigma, magnitude)))
