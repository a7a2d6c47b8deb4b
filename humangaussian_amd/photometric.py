"""The photometric loss of image fitting on the device: `photometric_loss` is L1 + D-SSIM and PSNR of a render against a
photograph in two HIP launches, its gradient with respect to the render in one (csrc/photometric.hip, include/hgs_rast.h:
hgs_photometric_forward / _backward state the formulas), and never waits on the host.  `l1_loss`, `ssim` and `psnr` are
drop-ins with the reference's signatures on the same kernels.

Reference:
  gaussiansplatting/utils/loss_utils.py    l1_loss, ssim / _ssim (11 taps, sigma 1.5, zero padding of 5)
  gaussiansplatting/utils/image_utils.py   psnr
  gaussiansplatting/train.py               loss = (1 - lambda_dssim) * Ll1 + lambda_dssim * (1 - ssim(image, gt_image))
Deviations: the gradient flows to the FIRST argument only (a second argument that requires grad is refused, not given a
silently partial gradient), and the window has 11 taps (any other window_size is refused).  There is no CPU path: tensors on
the CPU raise.  NaN or Inf in the inputs is outside the contract.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib

MAX_DIM = _lib.SI_MAX_DIM
MAX_PLANES = 65535
TILE_H, TILE_W = _lib.PM_TILE_H, _lib.PM_TILE_W     # pixels of one workgroup of the forward and of the backward
FINISH_CHUNK = _lib.PM_FINISH_CHUNK                 # the finalize step adds a plane's per-tile partials in strides of this
WINDOW_SIZE = len(_lib.PM_WINDOW)


class PhotometricLoss(NamedTuple):
    loss: torch.Tensor     # 0-dim: (1 - lambda_dssim) l1 + lambda_dssim (1 - ssim)
    l1: torch.Tensor       # 0-dim: mean |image - gt|
    ssim: torch.Tensor     # 0-dim: mean of the SSIM map
    psnr: torch.Tensor     # (C, 1) for a 3-D input, (B, 1) for a 4-D one; not differentiable


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, weight_l1, weight_dssim, psnr_per_plane, with_grad):
        loss, l1, ssim, ssim_image, sqerr, psnr, work = _lib.load_binding().photometric_forward(
            image, gt, weight_l1, weight_dssim, psnr_per_plane, with_grad)
        if with_grad:
            ctx.save_for_backward(image, gt, work)
        ctx.weights = (weight_l1, weight_dssim)
        ctx.mark_non_differentiable(sqerr, psnr)
        ctx.set_materialize_grads(False)      # an output the loss does not use arrives as None, not as zeros
        return loss, l1, ssim, ssim_image, sqerr, psnr

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim, g_ssim_image, _g_sqerr, _g_psnr):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        image, gt, work = ctx.saved_tensors

        def ready(g):      # an absent gradient stays None: the kernel takes a flag, not a zero tensor
            return None if g is None else g.detach().to(torch.float32).contiguous()

        d_image = _lib.load_binding().photometric_backward(image, gt, work, ctx.weights[0], ctx.weights[1], ready(g_loss),
                                                           ready(g_l1), ready(g_ssim), ready(g_ssim_image))
        return d_image, None, None, None, None, None


def _run(image, gt, lambda_dssim, names=("image", "gt")):
    """The checks of the contract and the one autograd node; returns its six outputs and whether the input was 3-D."""
    for t, name in zip((image, gt), names):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if image.dim() not in (3, 4):
        raise ValueError(f"{names[0]} must be (C, H, W) or (B, C, H, W), got {tuple(image.shape)}")
    if tuple(gt.shape) != tuple(image.shape):
        raise ValueError(f"{names[0]} {tuple(image.shape)} and {names[1]} {tuple(gt.shape)} differ in shape")
    if image.device != gt.device:
        raise ValueError(f"{names[0]} and {names[1]} must be on one device")
    if gt.requires_grad:
        raise ValueError(f"{names[1]} requires grad: the gradient flows to {names[0]} only (detach {names[1]}, or swap the arguments)")
    if not image.is_floating_point() or not gt.is_floating_point():
        raise ValueError(f"{names[0]} and {names[1]} must be floating-point tensors")
    lam = float(lambda_dssim)
    three_d = image.dim() == 3
    B, C, H, W = (1, *image.shape) if three_d else image.shape
    if B < 1 or C < 1 or H < 1 or W < 1 or H > MAX_DIM or W > MAX_DIM or B * C > MAX_PLANES or B * C * H * W >= 2 ** 31:
        raise ValueError(f"1..{MAX_PLANES} planes of 1..{MAX_DIM} pixels a side and fewer than 2^31 elements in all, "
                         f"got {tuple(image.shape)}")
    if image.device.type != "cuda":
        raise RuntimeError("humangaussian_amd: tensors must live on a HIP device (there is no CPU path)")
    image4 = image.to(torch.float32).reshape(B, C, H, W).contiguous()
    gt4 = gt.detach().to(torch.float32).reshape(B, C, H, W).contiguous()
    with_grad = torch.is_grad_enabled() and image4.requires_grad
    return _Photometric.apply(image4, gt4, 1.0 - lam, lam, three_d, with_grad), three_d


def photometric_loss(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2) -> PhotometricLoss:
    """image and gt (C, H, W) or (B, C, H, W) on a HIP device -> `PhotometricLoss`.  loss, l1 and ssim are 0-dim and
    differentiable with respect to image; psnr is not, and has the reference's shape: one value per channel of a 3-D
    input, per image of a 4-D one, `inf` where the two are identical."""
    (loss, l1, ssim_mean, _ssim_image, _sqerr, psnr_rows), _ = _run(image, gt, lambda_dssim)
    return PhotometricLoss(loss, l1, ssim_mean, psnr_rows.unsqueeze(1))


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """loss_utils.l1_loss: mean |network_output - gt|, differentiable with respect to network_output."""
    return _run(network_output, gt, 0.0, ("network_output", "gt"))[0][1]


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """loss_utils.ssim, differentiable with respect to img1: the mean of the SSIM map, or with size_average=False its
    mean per image, (B,), of a 4-D input (the reference's three mean(1) need four dimensions).  window_size is 11."""
    if window_size != WINDOW_SIZE:
        raise ValueError(f"window_size is {WINDOW_SIZE}: the kernel has the reference's default window only, got {window_size!r}")
    if not size_average and isinstance(img1, torch.Tensor) and img1.dim() != 4:
        raise ValueError(f"size_average=False needs a (B, C, H, W) input, got {tuple(img1.shape)}")
    out, _ = _run(img1, img2, 1.0, ("img1", "img2"))
    return out[2] if size_average else out[3]


def psnr(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """image_utils.psnr: 20 log10(1 / sqrt(mse)) with mse over `view(shape[0], -1)`, (shape[0], 1); not differentiable."""
    with torch.no_grad():
        out, _ = _run(img1, img2.detach() if isinstance(img2, torch.Tensor) else img2, 0.0, ("img1", "img2"))
    return out[5].unsqueeze(1)
