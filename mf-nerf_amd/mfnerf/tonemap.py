"""The HDR-NeRF tonemappers of the reference's exposure path (models/networks.py:81-94,111-132) on
the gfx950 kernels of csrc/tonemap.hip.

With rgb_act='None' the reference's rgb_net returns log-radiance, and one
tcnn.Network(1, 1, FullyFusedMLP ReLU/Sigmoid, 64 neurons, 1 hidden layer) per colour channel maps
log-radiance + log(exposure) to an LDR value.  tcnn pads each scalar to a 16-wide half row and runs
three 16 -> 64 -> 16 MLPs; here one launch takes the (n, C) log-radiance, adds the log-exposure and
evaluates the C networks per sample, and one deterministic launch pair gives the gradients
("Tonemapper semantics").  There is no CPU path: a CPU tensor raises.
"""
import torch

from ._lib import call, load, ptr, stream

N_PARAMS = 2048  # one tonemapper: W1 (64,16) row-major, then W2 (16,64) row-major (tcnn's layout)


def _exposure_arg(exposure, n, device):
    """(device f32 tensor or None, stride): None = unit exposure, one element = the same value for
    every sample (stride 0), n elements = per sample (stride 1)."""
    if exposure is None:
        return None, 0
    if not isinstance(exposure, torch.Tensor):
        exposure = torch.tensor(float(exposure), device=device)
    e = exposure.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if e.numel() == 1:
        return e, 0
    if e.numel() != n:
        raise RuntimeError(f"exposure has {e.numel()} values for {n} samples (expected 1 or {n})")
    return e, 1


def _check(lograd16, params, rgb16=None):
    n, C = lograd16.shape
    if C not in (1, 3):
        raise RuntimeError(f"tonemap: 1 or 3 channels, got {C}")
    if params.numel() != C * N_PARAMS:
        raise RuntimeError(f"tonemap: {C} channel(s) take {C * N_PARAMS} parameters, got {params.numel()}")
    if rgb16 is not None and rgb16.shape != lograd16.shape:
        raise RuntimeError("tonemap: rgb and log-radiance shapes differ")
    return n, C


def tonemap_fw(lograd16, exposure, e_stride, params):
    """mfnerf_tonemap_fw: lograd16 (n, C) f16, exposure None or device f32 read at [i * e_stride],
    params (C * 2048) f32 -> rgb (n, C) f16."""
    n, C = _check(lograd16, params)
    rgb = torch.empty(n, C, dtype=torch.float16, device=lograd16.device)
    call("mfnerf_tonemap_fw", ptr(lograd16), ptr(exposure), int(e_stride), n, C, ptr(params), ptr(rgb), stream())
    return rgb


def tonemap_bw(lograd16, exposure, e_stride, params, rgb16, dL_drgb):
    """mfnerf_tonemap_bw: -> dL_dlograd (n, C) f32, grad_params (C * 2048) f32; the same bits on every
    run (fixed-order reduction, no atomics)."""
    n, C = _check(lograd16, params, rgb16)
    dev = lograd16.device
    dx = torch.empty(n, C, dtype=torch.float32, device=dev)
    g = torch.empty(C * N_PARAMS, dtype=torch.float32, device=dev)
    ws = torch.empty(max(16, load().mfnerf_tonemap_bw_workspace(n, C)), dtype=torch.uint8, device=dev)
    call("mfnerf_tonemap_bw", ptr(lograd16), ptr(exposure), int(e_stride), n, C, ptr(params), ptr(rgb16),
         ptr(dL_drgb), ptr(dx), ptr(g), ptr(ws), stream())
    return dx, g


# ---------------------------------------------------------------- the fused training step's forms
def live_workspace(cap, device):
    """The backward's workspace for a capacity of `cap` samples (C = 3; any content)."""
    return torch.empty(max(16, load().mfnerf_tonemap_bw_workspace(cap, 3)), dtype=torch.uint8, device=device)


def tonemap_fw_live(lograd16, exposure_s, n_dev, params, rgb):
    """mfnerf_tonemap_fw_live: lograd16 (cap,3) f16, exposure_s (cap) f32 or None, n_dev (1) i32 on the
    device, params (3*2048) f32 -> rgb (cap,3) f32 (half values), rows below min(cap, *n_dev)."""
    call("mfnerf_tonemap_fw_live", ptr(lograd16), ptr(exposure_s), 0 if exposure_s is None else 1, lograd16.shape[0],
         ptr(n_dev), ptr(params), ptr(rgb), stream())
    return rgb


def tonemap_bw_live(lograd16, exposure_s, n_dev, params, rgb, dL_drgb, dL_dlograd, grad_params, workspace):
    """mfnerf_tonemap_bw_live into dL_dlograd (cap,3) f32 and grad_params (3*2048) f32 (overwritten)."""
    call("mfnerf_tonemap_bw_live", ptr(lograd16), ptr(exposure_s), 0 if exposure_s is None else 1, lograd16.shape[0],
         ptr(n_dev), ptr(params), ptr(rgb), ptr(dL_drgb), ptr(dL_dlograd), ptr(grad_params), ptr(workspace), stream())


def expand_exposure(exposure_ray, rays_a, n_dev, exposure_s):
    """mfnerf_expand_exposure (rendering.py:142-145): exposure_s[start:start+count] = exposure_ray[ray]
    per row (ray, start, count) of rays_a, below min(cap, *n_dev)."""
    call("mfnerf_expand_exposure", ptr(exposure_ray), ptr(rays_a), rays_a.shape[0], exposure_s.shape[0], ptr(n_dev),
         ptr(exposure_s), stream())
    return exposure_s


def unit_loss(params, target, grad_params, loss_out, amp=None):
    """mfnerf_tonemap_unit_loss (train.py:172-177), C = 3: loss_out (3) stored, its gradient added to
    grad_params (3*2048); amp: the step's mfnerf_amp_state (8 x i32) or None."""
    call("mfnerf_tonemap_unit_loss", ptr(params), 3, float(target), ptr(grad_params), ptr(loss_out), ptr(amp),
         stream())


def side_adam_step(params, grads, m, v, lr, betas, eps, step_dev, lr_dev=None, amp=None):
    """mfnerf_side_adam_step: Adam on a small parameter group with its own device step counter."""
    call("mfnerf_side_adam_step", ptr(params), ptr(grads), ptr(m), ptr(v), params.numel(), float(lr),
         float(betas[0]), float(betas[1]), float(eps), ptr(step_dev), ptr(lr_dev), ptr(amp), stream())


class TonemapFunction(torch.autograd.Function):
    """rgb (n, C) f16 = the C tonemappers of `params` (C * 2048 values, channel-major) on
    lograd (n, C) + log(exposure); exposure None, one value or one per sample.  The exposure gets no
    gradient; lograd's comes back in lograd's dtype."""

    @staticmethod
    def forward(ctx, lograd, exposure, params):
        if not lograd.is_cuda or not params.is_cuda:
            raise RuntimeError("mfnerf.tonemap: the tonemappers run on the GPU only (HIP kernels; no CPU path)")
        if lograd.dim() != 2:
            raise RuntimeError("tonemap: log-radiance must be (n, C)")
        l16 = lograd.detach().half().contiguous()
        p32 = params.detach().float().contiguous().reshape(-1)
        e, e_stride = _exposure_arg(exposure, l16.shape[0], l16.device)
        rgb = tonemap_fw(l16, e, e_stride, p32)
        ctx.save_for_backward(l16, p32, rgb, *([] if e is None else [e]))
        ctx.e_stride, ctx.x_dtype, ctx.p_dtype, ctx.p_shape = e_stride, lograd.dtype, params.dtype, params.shape
        return rgb

    @staticmethod
    def backward(ctx, dout):
        l16, p32, rgb = ctx.saved_tensors[:3]
        e = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        dx, g = tonemap_bw(l16, e, ctx.e_stride, p32, rgb, dout.float().contiguous())
        return dx.to(ctx.x_dtype), None, g.to(ctx.p_dtype).reshape(ctx.p_shape)
