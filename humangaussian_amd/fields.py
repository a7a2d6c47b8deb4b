"""A trained avatar as a triangle mesh, on the GPU: the density field of the Gaussians on a regular grid and its
iso-surface - `GaussianModel.extract_fields` / `extract_mesh` of the reference (/root/reference/gs_renderer.py:240-361:
a Python loop over 16^3 blocks there, then `mcubes.marching_cubes` on the CPU).

HIP kernels: csrc/fields.hip through `hgs_field_*` / `hgs_mc_*` of the C ABI (include/hgs_rast.h states the semantics:
the opacity cut, the normalisation, the per-block cut of the sum, the inside rule and the winding of the surface).
The field is bit-reproducible from call to call.  No CPU path: CPU tensors raise.  The reference's `clean_mesh` /
`decimate_mesh` (kiui + pymeshlab, CPU) are not part of this module."""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib

OPACITY_CUT = 0.005


def _model_tensors(model):
    if isinstance(model, (tuple, list)):
        if len(model) != 4:
            raise ValueError("extract_fields: tensors are (xyz (P,3), opacity (P,1), scaling (P,3), rotation (P,4))")
        return tuple(model), False
    return (model.get_xyz, model.get_opacity, model.get_scaling, model._rotation), True


def _check_device(tensors, what):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"humangaussian_amd: {what} needs tensors on a HIP device (torch device type 'cuda'), got "
                               f"{getattr(t, 'device', type(t))}; there is no CPU path")


def extract_fields(model_or_tensors, resolution: int = 128, num_blocks: int = 16, relax_ratio: float = 1.5,
                   return_block_counts: bool = False):
    """occ (resolution,)*3 fp32 on the device: occ[p] = sum of opacity * exp(-1/2 d^T Sigma^-1 d) over the Gaussians of
    p's block (those with opacity > 0.005 whose normalised centre lies strictly inside the block's sample box grown by
    relax_ratio * 2 / num_blocks), sampled at linspace(-1, 1, resolution)^3 of the normalised cloud.

    `model_or_tensors`: the reference's GaussianModel (anything with get_xyz, get_opacity, get_scaling, _rotation); its
    `center` (tensor) and `scale` (float) are set as the reference does and `occ` is returned.  Or the four tensors
    (xyz, opacity, scaling, rotation) - activated opacities and scales, the raw quaternion: returns (occ, center, scale).
    return_block_counts appends the (num_blocks,)*3 int32 tensor of the blocks' list lengths.
    resolution must be a multiple of num_blocks, num_blocks <= 32 and resolution / num_blocks <= 256.
    No Gaussian above the opacity cut: a zero field, center 0 and scale 1.  Finding that out takes the plan's four small
    kernels and its one host wait (the filter runs on the device); only the lists and the evaluation are not launched.
    With no Gaussian at all (P == 0) nothing is launched."""
    if num_blocks < 1:
        raise ValueError(f"extract_fields: num_blocks ({num_blocks}) must be at least 1")
    if resolution % num_blocks != 0:
        raise ValueError(f"extract_fields: resolution ({resolution}) must be a multiple of num_blocks ({num_blocks})")
    block_size = 2 / num_blocks
    (xyz, opacity, scaling, rotation), is_model = _model_tensors(model_or_tensors)
    _check_device((xyz, opacity, scaling, rotation), "extract_fields")
    dev = xyz.device
    counts = None
    if xyz.shape[0] == 0:
        occ, geo = torch.zeros([resolution] * 3, dtype=torch.float32, device=dev), None
        if return_block_counts:
            counts = torch.zeros([num_blocks] * 3, dtype=torch.int32, device=dev)
    else:
        with torch.no_grad():
            axis = torch.linspace(-1, 1, resolution).to(dev)      # the reference's sample positions, bit for bit
            occ, counts, geo, sizes = _lib.load_binding().field_extract(
                xyz.detach(), opacity.detach().reshape(-1), scaling.detach(), rotation.detach(), axis, num_blocks,
                block_size * relax_ratio, return_block_counts)
        if sizes[0] == 0:
            geo = None
    if geo is None:
        center, scale = torch.zeros(3, dtype=torch.float32, device=dev), 1.0
    else:
        center = torch.tensor(geo[:3], dtype=torch.float32, device=dev)
        scale = 1.8 / geo[3] if geo[3] > 0 else float("inf")
    if is_model:
        model_or_tensors.center, model_or_tensors.scale = center, scale
        return (occ, counts) if return_block_counts else occ
    return (occ, center, scale, counts) if return_block_counts else (occ, center, scale)


def marching_cubes(occ: torch.Tensor, threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(vertices (V,3) fp32, triangles (T,3) int32) of the iso-surface of a field (X,Y,Z).  `mcubes.marching_cubes`'
    conventions for the coordinates (index units), the interpolation (linear along the crossed grid edge) and the inside
    rule (value >= threshold); the case table is this project's own (csrc/mc_table.h), so the triangle list is not
    mcubes' triangle for triangle.  One vertex per crossed edge, shared by its triangles; normals point from high values
    to low.  A field with a dimension of size 1 has no cell: (0,3) and (0,3)."""
    _check_device((occ,), "marching_cubes")
    if occ.dim() != 3:
        raise ValueError(f"marching_cubes: the field must be (X, Y, Z), got {tuple(occ.shape)}")
    return _lib.load_binding().marching_cubes(occ.detach(), float(threshold))


def extract_mesh(model, density_thresh: float = 1, resolution: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """(vertices (V,3) fp32 in world space, faces (T,3) int32) of the avatar's density iso-surface: the reference's
    extract_mesh up to (not including) clean_mesh / decimate_mesh."""
    if isinstance(model, (tuple, list)):
        occ, center, scale = extract_fields(model, resolution)
    else:
        occ = extract_fields(model, resolution)
        center, scale = model.center, model.scale
    vertices, triangles = marching_cubes(occ, density_thresh)
    vertices = vertices / (resolution - 1.0) * 2 - 1
    vertices = vertices / scale + center
    return vertices, triangles
