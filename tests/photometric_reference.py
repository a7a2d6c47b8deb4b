"""The photometric loss as plain torch ops under autograd: the formulas of include/hgs_rast.h (hgs_photometric_*), which are
those of the reference's image-fitting step (gaussiansplatting/utils/loss_utils.py: l1_loss, ssim / _ssim;
utils/image_utils.py: psnr; train.py: the weighted sum).  Run in float64 it is the truth the kernels are compared with, in
float32 on the CPU the yardstick: a kernel's distance from the float64 run may be 4 x the float32 run's own on the same
input (the kernel adds the 121 taps row by row, this file multiplies by the 2-D window as the reference does), with the
floors of `gates` below.

  formulas(image, gt, lam)            loss, l1, ssim, ssim_image, psnr - differentiable, any dtype, 3-D or 4-D input
  derivative_maps / filtered_gradient the header's backward formula spelled out (no autograd): the adjoint argument
  content_case / CONTENT_KINDS        the inputs of tests/test_gpu_photometric.py
  grad_distance, gates                the measures and the gates of the GPU tests
"""
from math import exp

import torch
import torch.nn.functional as F

WINDOW_SIZE, SIGMA, PAD = 11, 1.5, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window1d():
    """The 11 fp32 taps: exp(-(i - 5)^2 / (2 sigma^2)) in double, rounded to fp32, normalised in fp32."""
    g = torch.tensor([exp(-(i - WINDOW_SIZE // 2) ** 2 / float(2 * SIGMA ** 2)) for i in range(WINDOW_SIZE)], dtype=torch.float32)
    return g / g.sum()


def window2d(channels, dtype):
    """(channels, 1, 11, 11): the outer product of the taps rounded to fp32, then cast - what every dtype is filtered with."""
    w = window1d().unsqueeze(1)
    return w.mm(w.t()).to(dtype).expand(channels, 1, WINDOW_SIZE, WINDOW_SIZE).contiguous()


def filt(v, win):
    return F.conv2d(v, win, padding=PAD, groups=v.shape[-3])


def moments(x, y):
    win = window2d(x.shape[-3], x.dtype).to(x.device)
    mu1, mu2 = filt(x, win), filt(y, win)
    return mu1, mu2, filt(x * x, win) - mu1 * mu1, filt(y * y, win) - mu2 * mu2, filt(x * y, win) - mu1 * mu2


def ssim_map(x, y):
    mu1, mu2, s1, s2, s12 = moments(x, y)
    return ((2 * (mu1 * mu2) + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def psnr(x, y):
    mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def formulas(image, gt, lam=0.2):
    """image, gt: (C, H, W) or (B, C, H, W) of one dtype.  ssim_image is None for a 3-D input."""
    smap = ssim_map(image, gt)
    l1 = (image - gt).abs().mean()
    ssim = smap.mean()
    out = {"l1": l1, "ssim": ssim, "loss": (1.0 - lam) * l1 + lam * (1.0 - ssim),
           "ssim_image": smap.mean(1).mean(1).mean(1) if image.dim() == 4 else None,
           "psnr": psnr(image.detach(), gt.detach())}
    return out


def run(image, gt, dtype, lam=0.2):
    """formulas in dtype on copies of the fp32 inputs, and the gradient of the loss with respect to image."""
    x = image.detach().to(dtype).requires_grad_(True)
    out = formulas(x, gt.detach().to(dtype), lam)
    out["grad"], = torch.autograd.grad(out["loss"], x, retain_graph=True)
    out["grad_l1"], = torch.autograd.grad(out["l1"], x, retain_graph=True)
    out["grad_ssim"], = torch.autograd.grad(out["ssim"], x)
    return {k: (v.detach() if v is not None else None) for k, v in out.items()}


def derivative_maps(x, y):
    """The three maps the forward leaves for the backward (header: dS/dmu1 total, dS/ds1, dS/ds12)."""
    mu1, mu2, s1, s2, s12 = moments(x, y)
    A1, A2 = 2 * (mu1 * mu2) + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    S = (A1 * A2) / (B1 * B2)
    return 2 * (mu2 * (A2 - A1) + mu1 * S * (B1 - B2)) / (B1 * B2), -S / B2, 2 * A1 / (B1 * B2)


def filtered_gradient(x, y, g_ssim, g_l1):
    """The header's backward for d(g_ssim ssim + g_l1 l1)/dx, 4-D input: the window is symmetric, so the adjoint of the
    zero-padded filter is the same zero-padded filter applied to the derivative maps."""
    dmu, ds1, ds12 = derivative_maps(x, y)
    win = window2d(x.shape[-3], x.dtype).to(x.device)
    n = x.numel()
    return g_ssim / n * (filt(dmu, win) + 2 * x * filt(ds1, win) + y * filt(ds12, win)) + g_l1 / n * torch.sign(x - y)


CONTENT_KINDS = ("random", "smooth", "constant_equal", "one_vs_zero", "near_equal", "half_equal", "out_of_range")


def content_case(kind, B, C, H, W, seed=0):
    """(image, gt), fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, C, H, W)
    if kind == "random":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if kind == "smooth":
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        ch = torch.arange(1, C + 1, dtype=torch.float32).view(1, C, 1, 1) / C
        gt = (0.15 + 0.7 * (0.5 * (xx + yy)) * ch).expand(shape).contiguous()
        return gt + 0.01 * torch.randn(shape, generator=g), gt
    if kind == "constant_equal":
        return torch.full(shape, 0.5), torch.full(shape, 0.5)
    if kind == "one_vs_zero":
        return torch.ones(shape), torch.zeros(shape)
    if kind == "near_equal":
        gt = torch.rand(shape, generator=g)
        return gt + 1e-4 * torch.randn(shape, generator=g), gt
    if kind == "half_equal":
        gt = torch.rand(shape, generator=g)
        other = torch.rand(shape, generator=g)
        return torch.where(torch.rand(shape, generator=g) < 0.5, gt, other), gt
    if kind == "out_of_range":
        return 1.5 * torch.randn(shape, generator=g) - 0.25, 2.0 * torch.rand(shape, generator=g) - 1.0
    raise ValueError(kind)


SCALAR_FLOOR, GRAD_FLOOR, MARGIN = 1e-6, 1e-5, 4.0


def grad_distance(g, g64):
    """max |g - g64| / max(max |g64|, 1 / numel): the second term keeps a case whose true gradient vanishes meaningful."""
    g64 = g64.double()
    return float((g.double().cpu() - g64).abs().max() / max(float(g64.abs().max()), 1.0 / g64.numel()))


def scalar_distance(v, v64):
    """|v - v64| relative to max(1, |v64|): loss, l1 and ssim are below 1 in size, psnr is tens of dB; inf == inf is 0."""
    v, v64 = v.double().cpu().reshape(-1), v64.double().reshape(-1)
    same_inf = torch.isinf(v) & torch.isinf(v64) & (v == v64)
    d = torch.where(same_inf, torch.zeros_like(v), (v - v64).abs() / v64.abs().clamp(min=1.0))
    return float(d.max())


def gates(r32, r64):
    """The gates of one input from the distance of the fp32 run of this file from its fp64 run: margin 4, with floors."""
    g = {k: max(MARGIN * scalar_distance(r32[k], r64[k]), SCALAR_FLOOR) for k in ("loss", "l1", "ssim", "ssim_image", "psnr")
         if r64[k] is not None}
    for k in ("grad", "grad_l1", "grad_ssim"):
        g[k] = max(MARGIN * grad_distance(r32[k], r64[k]), GRAD_FLOOR)
    return g
