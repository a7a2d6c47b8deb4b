"""fp64 reference of the antialiasing filter (HGS_ANTIALIAS): upstream 3DGS's screen-space filter from Mip-Splatting.

The oracle's preprocess is wrapped, not changed: its opacity is multiplied by
    rho = sqrt(max(2.5e-5, det(cov2D - 0.3 I) / det(cov2D)))
computed in torch from pre["cov2D"] (a, b, c WITH the 0.3 px^2 dilation), so autograd supplies the reference gradients.
`antialiased()` installs the wrapper (unittest.mock.patch.object) around oracle.rasterize / oracle.forward_backward."""
import contextlib
from unittest import mock

import torch

import oracle
from oracle import gs_oracle

MIN_RATIO = 2.5e-5
_preprocess = gs_oracle.preprocess


def rho_of(cov2D):
    """rho per Gaussian from the dilated (a, b, c); Gaussians with det == 0 (culled) get rho = 1."""
    a, b, c = cov2D.unbind(1)
    h = gs_oracle.LOWPASS
    det = a * c - b * b
    ok = det != 0
    det_safe = torch.where(ok, det, torch.ones_like(det))
    ratio = ((a - h) * (c - h) - b * b) / det_safe
    return torch.where(ok, torch.sqrt(torch.clamp(ratio, min=MIN_RATIO)), torch.ones_like(det))


def preprocess_aa(*args, **kwargs):
    pre = dict(_preprocess(*args, **kwargs))
    pre["rho"] = rho_of(pre["cov2D"])
    pre["opacity"] = pre["opacity"] * pre["rho"]
    return pre


@contextlib.contextmanager
def antialiased():
    with mock.patch.object(gs_oracle, "preprocess", preprocess_aa):
        yield


def rasterize(*args, **kwargs):
    with antialiased():
        return oracle.rasterize(*args, **kwargs)


def forward_backward(*args, **kwargs):
    with antialiased():
        return oracle.forward_backward(*args, **kwargs)


# ------------------------------------------------------------------- what the filter is for: one scene, two resolutions
FILTER_SCENE = dict(P=300, sh_degree=0, seed=7, spread=0.45, scale=0.0025, dist=2.0, fovy=50.0)
FILTER_HI, FILTER_LO = 1024, 256


def filter_scene(H):
    """A fixed sparse scene of small, semi-transparent Gaussians seen at H x H: ~1.4 px at 1024^2, ~0.35 px at 256^2."""
    from helpers import make_scene
    sc = make_scene(H=H, W=H, **FILTER_SCENE)
    g = torch.Generator().manual_seed(11)
    sc["opacities"] = 0.2 + 0.4 * torch.rand(sc["opacities"].shape, generator=g)
    return sc


def pooled_alpha_error(alpha_hi, alpha_lo):
    """mean |alpha at the low resolution - 4x4 average pool of alpha at the high one|"""
    f = FILTER_HI // FILTER_LO
    pooled = torch.nn.functional.avg_pool2d(alpha_hi.reshape(1, 1, FILTER_HI, FILTER_HI).double(), f)
    return float((alpha_lo.reshape(1, 1, FILTER_LO, FILTER_LO).double() - pooled).abs().mean())


def filter_error_ratio_fp64():
    """error with the filter / error without it, fp64 reference (the number test_gpu_antialias.py commits)."""
    from helpers import oracle_settings
    errs = {}
    for aa in (False, True):
        alphas = []
        for H in (FILTER_HI, FILTER_LO):
            sc = filter_scene(H)
            args = (sc["means3D"].double(), None, sc["shs"].double(), None, sc["opacities"].double(), sc["scales"].double(),
                    sc["rotations"].double(), None, oracle_settings(sc))
            with torch.no_grad():
                out = rasterize(*args, dtype=torch.float64) if aa else oracle.rasterize(*args, dtype=torch.float64)
            alphas.append(out[3])
        errs[aa] = pooled_alpha_error(*alphas)
    return errs[True] / errs[False], errs
