"""torch.autograd face of the ray bundles: radiance of caller-given rays as a differentiable function of the Gaussians.

    L = radiance_rays(renderer, mu, albedo, sigma, magnitude, origins, dirs)      # [nrays, 4], on cuda
    loss(L).backward()                                                            # mu.grad, albedo.grad, sigma.grad, magnitude.grad

Forward is Renderer.radiance_rays_device, backward Renderer.radiance_rays_grad_device (include/vrt_hip.h, "gradient bundles"): the
derivative with each ray's kept list held fixed, under {vcl_exp, expf} x {A&S erf, erff} only, summed with float atomics (not bitwise
reproducible).  No gradient is returned for the rays.

A Gaussian whose magnitude is exactly 0 is dropped by every ray's cull and therefore receives NO gradient, magnitude.grad included
(although the true derivative is not 0): initialise magnitudes away from 0.

Known limit: the scene reaches the renderer through the HOST -- forward copies the four parameter tensors to the CPU and calls
set_gaussians_soa, which waits for the device and rebuilds the scene tables.  A device-side scene update is not part of this
library yet; a fitting loop pays that upload once per step.
"""
import numpy as np
import torch

from . import GRAD_STRIDE, grad_columns


class _RadianceRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, renderer, mu, albedo, sigma, magnitude, origins, dirs):
        dev = torch.device("cuda", torch.cuda.current_device())
        host = [t.detach().to("cpu", torch.float32).contiguous().numpy() for t in (mu, albedo, sigma, magnitude)]
        renderer.set_gaussians_soa(host[0], host[1][:, :3], host[2], host[3], alpha=np.ascontiguousarray(host[1][:, 3]))
        o = origins.detach().to(dev, torch.float32).contiguous()
        d = dirs.detach().to(dev, torch.float32).contiguous().reshape(-1, 3)
        per_ray = o.numel() != 3
        out = torch.empty((d.shape[0], 4), dtype=torch.float32, device=dev)
        if d.shape[0]:
            renderer.radiance_rays_device(d.shape[0], o.data_ptr(), per_ray, d.data_ptr(), d_radiance=out.data_ptr(),
                                          stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.renderer, ctx.rays, ctx.n = renderer, (o, d, per_ray), len(host[2])
        ctx.devices = [t.device for t in (mu, albedo, sigma, magnitude)]
        ctx.dtypes = [t.dtype for t in (mu, albedo, sigma, magnitude)]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        o, d, per_ray = ctx.rays
        g = grad_out.to(o.device, torch.float32).contiguous()
        table = torch.zeros((ctx.n, GRAD_STRIDE), dtype=torch.float32, device=o.device)
        if d.shape[0] and ctx.n:
            ctx.renderer.radiance_rays_grad_device(d.shape[0], o.data_ptr(), per_ray, d.data_ptr(), g.data_ptr(), table.data_ptr(),
                                                   stream=torch.cuda.current_stream(o.device).cuda_stream)
        cols = grad_columns(table)
        grads = [cols[k].to(dev, dt) for k, dev, dt in zip(("mu", "albedo", "sigma", "magnitude"), ctx.devices, ctx.dtypes)]
        return (None, *grads, None, None)


def radiance_rays(renderer, mu, albedo, sigma, magnitude, origins, dirs):
    """Radiance [nrays, 4] (a cuda tensor on torch's current device and stream) of the rays through the scene of the four parameter
    tensors mu [N, 3], albedo [N, 4], sigma [N], magnitude [N], differentiable in those four.  origins: [3] or [nrays, 3]; dirs:
    [nrays, 3], unit length.  The scene of `renderer` is REPLACED by the parameters, through the host (see the module's docstring);
    backward must run before the renderer's scene or options change again."""
    return _RadianceRays.apply(renderer, mu, albedo, sigma, magnitude, origins, dirs)
