"""The stretch between `render_views()` and the diffusion guidance on the device: `guidance_images` turns the batched
rasterizer outputs into the two images the guidance is handed and the two opacity losses, differentiable with respect to
both inputs, in three HIP launches forward and three backward (csrc/step_images.hip, include/hgs_rast.h:
hgs_step_images_forward / _backward state the formulas) and never waits on the host.

Reference:
  threestudio/systems/GaussianDreamer.py:285-302   stack the views, opacity = depths / (depths.max() + 1e-5)
  threestudio/systems/GaussianDreamer.py:330-333   per-view amin / amax of the depth, normalise, repeat to 3 channels
  threestudio/models/guidance/dual_branch_guidance.py:762-770   F.interpolate(..., "bilinear", align_corners=False), the cast
  threestudio/systems/GaussianDreamer.py:359-366   loss_sparsity, loss_opaque
There is no CPU path: tensors on the CPU raise.  NaN or Inf in the inputs is outside the contract.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import torch

from . import _lib

MAX_DIM = _lib.SI_MAX_DIM


class StepImages(NamedTuple):
    rgb: torch.Tensor                # (B, 3, h, w): the bilinear resize of the colour
    depth: torch.Tensor              # (B, 3, h, w): the resize of the per-view normalised depth, three times
    loss_sparsity: torch.Tensor      # 0-dim: mean sqrt(opacity^2 + 0.01)
    loss_opaque: torch.Tensor        # 0-dim: binary cross entropy of the clamped opacity with itself
    depth_min: torch.Tensor          # (B,)   not differentiable
    depth_max: torch.Tensor          # (B,)   not differentiable
    depth_global_max: torch.Tensor   # 0-dim  not differentiable


class _StepImages(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, depth, h, w, half_images):
        rgb, depth3, ls, lo, dmin, dmax, gmax, counts = _lib.load_binding().step_images_forward(render, depth, h, w, half_images)
        ctx.save_for_backward(depth, dmin, dmax, gmax, counts)
        ctx.size = (h, w, half_images)
        ctx.mark_non_differentiable(dmin, dmax, gmax)
        ctx.set_materialize_grads(False)      # an output the loss does not use arrives as None, not as zeros
        return rgb, depth3, ls, lo, dmin, dmax, gmax

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_ls, g_lo, _gmin, _gmax, _gg):
        depth, dmin, dmax, gmax, counts = ctx.saved_tensors
        h, w, half_images = ctx.size
        idt = torch.float16 if half_images else torch.float32

        def ready(g, dt):      # an absent gradient stays None: the kernels take a flag, not a zero tensor
            return None if g is None else g.detach().to(dt).contiguous()

        need_render, need_depth = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_render, d_depth = _lib.load_binding().step_images_backward(
            depth, dmin, dmax, gmax, counts, h, w, half_images,
            ready(g_rgb, idt) if need_render else None,
            ready(g_depth, idt) if need_depth else None,
            ready(g_ls, torch.float32) if need_depth else None,
            ready(g_lo, torch.float32) if need_depth else None)
        return d_render, d_depth, None, None, None


def guidance_images(render: torch.Tensor, depth: torch.Tensor, size: Tuple[int, int] = (512, 512),
                    dtype: torch.dtype = torch.float32) -> StepImages:
    """render (B, 3, H, W) and depth (B, 1, H, W), fp32 on a HIP device (`render_views` stacked) -> `StepImages` at
    `size` = (h, w) with 1 <= h <= H and 1 <= w <= W (the same size or smaller; pass (H, W) when the guidance should
    resize itself).  dtype (torch.float32 or torch.float16) is that of the two images and of their incoming gradients:
    the kernels compute in fp32 and round once.  Differentiable with respect to render and depth; depth_min, depth_max
    and depth_global_max are not.  Hand the images to the guidance as `rgb.permute(0, 2, 3, 1)` (a view)."""
    for t, name in ((render, "render"), (depth, "depth")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("dtype is torch.float32 or torch.float16")
    if render.dim() != 4 or render.shape[1] != 3:
        raise ValueError(f"render must be (B, 3, H, W), got {tuple(render.shape)}")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"depth must be (B, 1, H, W), got {tuple(depth.shape)}")
    B, _, H, W = render.shape
    if tuple(depth.shape) != (B, 1, H, W):
        raise ValueError(f"render {tuple(render.shape)} and depth {tuple(depth.shape)} differ in B, H or W")
    if render.device != depth.device:
        raise ValueError("render and depth must be on one device")
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size is (h, w), got {size!r}") from None
    if B < 1 or H < 1 or W < 1 or H > MAX_DIM or W > MAX_DIM or B * H * W >= 2 ** 31 or B > 65535:
        raise ValueError(f"1..65535 views of 1..{MAX_DIM} pixels a side and fewer than 2^31 pixels in all, got {tuple(render.shape)}")
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"size {(h, w)} must be within [1, {H}] x [1, {W}]: the same size or downsampling, upsampling is refused")
    if render.device.type != "cuda":
        raise RuntimeError("humangaussian_amd: tensors must live on a HIP device (there is no CPU path)")
    render = render.to(torch.float32).contiguous()
    depth = depth.to(torch.float32).contiguous()
    return StepImages(*_StepImages.apply(render, depth, h, w, dtype == torch.float16))
