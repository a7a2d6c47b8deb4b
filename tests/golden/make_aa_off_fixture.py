"""Generates tests/golden/aa_off_parent.json: fingerprints (sha256 of the raw bytes) of the outputs, radii and every
gradient of three small rasterizer calls WITHOUT the antialiasing keyword - one view (SH 2), three views in one batched
call (SH 1), one view with fused activations (SH 0) - made by the build of the commit BEFORE the antialiasing filter
(ABI 16).  Run on a GPU box from a checkout of that commit, with this file copied in:

    python tests/golden/make_aa_off_fixture.py OUT.json

tests/test_gpu_antialias.py::test_off_path_equals_the_parent_commit recomputes them with `fingerprints()` and requires
the same bits: the filter, off, changes nothing.  Only API that both commits have is used."""
import hashlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers import make_scene  # noqa: E402
from humangaussian_amd import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians_batch, synth  # noqa: E402
from humangaussian_amd import rasterizer as R  # noqa: E402

DEV = "cuda"
NAMES = ("means3D", "shs", "opacities", "scales", "rotations")


def _h(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _settings(sc, cam):
    return GaussianRasterizationSettings(cam.image_height, cam.image_width, math.tan(cam.FoVx * 0.5),
                                         math.tan(cam.FoVy * 0.5), sc["bg"].to(DEV), 1.0,
                                         cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV),
                                         sc["sh_degree"], cam.camera_center.to(DEV), False, False)


def _weights(lead, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(lead + s, generator=g).to(DEV) for s in ((3, H, W), (1, H, W), (1, H, W))]


def _record(out, name, outs, ins, m2):
    for k, t in zip(("color", "radii", "depth", "alpha"), outs):
        out[f"{name}/{k}"] = _h(t)
    for k in NAMES:
        out[f"{name}/grad_{k}"] = _h(ins[k].grad)
    out[f"{name}/grad_means2D"] = _h(m2.grad)


def fingerprints():
    out = {}
    H, W = 48, 64
    # one view, SH 2, through GaussianRasterizer
    sc = make_scene(P=600, sh_degree=2, seed=81, H=H, W=W, spread=0.3)
    ins = {k: sc[k].to(DEV).requires_grad_(True) for k in NAMES}
    m2 = torch.zeros_like(ins["means3D"], requires_grad=True)
    c, r, d, a = GaussianRasterizer(_settings(sc, sc["cam"]))(means3D=ins["means3D"], means2D=m2, shs=ins["shs"],
                                                              opacities=ins["opacities"], scales=ins["scales"],
                                                              rotations=ins["rotations"])
    torch.autograd.backward([c, d, a], _weights((), H, W, 1))
    _record(out, "single_sh2", (c, r, d, a), ins, m2)
    # three views in one batched call, SH 1
    sc = make_scene(P=600, sh_degree=1, seed=82, H=H, W=W, spread=0.3)
    cams = [synth.orbit_camera(10.0 * i, -150 + 100 * i, 1.8 + 0.3 * i, 50.0, H, W) for i in range(3)]
    ins = {k: sc[k].to(DEV).requires_grad_(True) for k in NAMES}
    m2 = torch.zeros((3,) + tuple(ins["means3D"].shape), device=DEV, requires_grad=True)
    c, r, d, a = rasterize_gaussians_batch(ins["means3D"], m2, ins["shs"], None, ins["opacities"], ins["scales"],
                                           ins["rotations"], None, [_settings(sc, cm) for cm in cams])
    torch.autograd.backward([c, d, a], _weights((3,), H, W, 2))
    _record(out, "batch3_sh1", (c, r, d, a), ins, m2)
    # one view, SH 0, fused activations on the raw parameters
    sc = make_scene(P=600, sh_degree=0, seed=83, H=H, W=W, spread=0.3)
    raw = dict(means3D=sc["means3D"], shs=sc["shs"], opacities=torch.logit(sc["opacities"]),
               scales=torch.log(sc["scales"]), rotations=sc["rotations"] * 1.7)
    ins = {k: v.to(DEV).requires_grad_(True) for k, v in raw.items()}
    m2 = torch.zeros((1,) + tuple(ins["means3D"].shape), device=DEV, requires_grad=True)
    c, r, d, a = rasterize_gaussians_batch(ins["means3D"], m2, ins["shs"], None, ins["opacities"], ins["scales"],
                                           ins["rotations"], None, [_settings(sc, sc["cam"])],
                                           activation_flags=R.ACT_OPACITY_SIGMOID | R.ACT_SCALE_EXP
                                           | R.ACT_ROTATION_NORMALIZE)
    torch.autograd.backward([c, d, a], _weights((1,), H, W, 3))
    _record(out, "fused_sh0", (c, r, d, a), ins, m2)
    return out


if __name__ == "__main__":
    fp = fingerprints()
    with open(sys.argv[1], "w") as f:
        json.dump(fp, f, indent=1, sort_keys=True)
    print(f"wrote {len(fp)} fingerprints to {sys.argv[1]}")
