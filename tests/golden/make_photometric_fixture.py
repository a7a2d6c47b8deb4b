"""Generates tests/golden/photometric_reference.npz: the reference's own `l1_loss`, `ssim`
(/root/reference/gaussiansplatting/utils/loss_utils.py) and `psnr` (utils/image_utils.py) run on the CPU in float64 and in
float32 on a handful of small inputs - the loss at lambda_dssim = 0.2 as train.py forms it, ssim with size_average True and
False, psnr under its 3-D and 4-D shape rules, and the autograd gradient of the loss with respect to the first image.
Run in the build container (imports /root/reference, which does not exist on the GPU box):

    python tests/golden/make_photometric_fixture.py

Only arrays are stored.  tests/test_photometric_cpu.py holds the restatement (tests/photometric_reference.py) against them."""
import os
import sys

import numpy as np
import torch

REF = "/root/reference/gaussiansplatting"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REF, os.path.join(ROOT, "tests")]

from utils.image_utils import psnr  # noqa: E402
from utils.loss_utils import l1_loss, ssim  # noqa: E402
import photometric_reference as PR  # noqa: E402

LAMBDA = 0.2
# name: (kind, shape, seed); a 3-tuple shape is a 3-D input
CASES = {
    "random": ("random", (2, 3, 19, 23), 1),
    "smooth": ("smooth", (1, 2, 37, 53), 2),
    "near_equal": ("near_equal", (1, 3, 16, 17), 3),
    "chw": ("random", (3, 12, 16), 4),
    "tiny": ("out_of_range", (1, 1, 5, 7), 5),
}


def inputs(name):
    kind, shape, seed = CASES[name]
    x, y = PR.content_case(kind, *((1,) + shape if len(shape) == 3 else shape), seed=seed)
    return (x[0], y[0]) if len(shape) == 3 else (x, y)


def record(x, y, dtype):
    img = x.to(dtype).requires_grad_(True)
    gt = y.to(dtype)
    l1 = l1_loss(img, gt)
    s = ssim(img, gt)
    loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - s)
    grad, = torch.autograd.grad(loss, img)
    out = {"loss": loss, "l1": l1, "ssim": s, "psnr": psnr(img, gt), "grad": grad}
    if img.dim() == 4:
        out["ssim_image"] = ssim(img, gt, size_average=False)
    return {k: v.detach().numpy() for k, v in out.items()}


def main():
    arrays = {}
    for name in CASES:
        x, y = inputs(name)
        arrays[f"{name}/image"], arrays[f"{name}/gt"] = x.numpy(), y.numpy()
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            for k, v in record(x, y, dtype).items():
                arrays[f"{name}/{tag}/{k}"] = v
        g64, g32 = arrays[f"{name}/f64/grad"], arrays[f"{name}/f32/grad"]
        print("%-10s loss %.9f  fp32 - fp64: loss %.2e  max|dg|/max|g| %.2e" % (
            name, arrays[f"{name}/f64/loss"], abs(float(arrays[f"{name}/f32/loss"]) - float(arrays[f"{name}/f64/loss"])),
            np.abs(g32 - g64).max() / np.abs(g64).max()))
    path = os.path.join(ROOT, "tests", "golden", "photometric_reference.npz")
    np.savez_compressed(path, lambda_dssim=np.float64(LAMBDA), **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
