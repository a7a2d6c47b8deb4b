"""A trained avatar as a triangle mesh, on the GPU: the density field of the Gaussians on a regular grid and its
iso-surface - `GaussianModel.extract_fields` / `extract_mesh` of the reference (/root/reference/gs_renderer.py:240-361:
a Python loop over 16^3 blocks there, then `mcubes.marching_cubes` on the CPU).

HIP kernels: csrc/fields.hip through `hgs_field_*` / `hgs_mc_*` of the C ABI (include/hgs_rast.h states the semantics:
the opacity cut, the normalisation, the per-block cut of the sum, the inside rule and the winding of the surface).
The field is bit-reproducible from call to call.  `GaussianField` keeps a field's plan and lists and evaluates it at
arbitrary points (`hgs_fsample`: density, outward normal, opacity-weighted colour) - the vertex attributes of
`extract_mesh_attributes`, an extension the reference has no counterpart for.  No CPU path: CPU tensors raise.  The reference's `clean_mesh` /
`decimate_mesh` (kiui + pymeshlab, CPU) are not reproduced; `extract_clean_mesh(clean=True, decimate_target=...)` finishes the
mesh on the device with meshclean.py's component filter and vertex clustering instead."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .meshclean import MIN_D, MIN_F, clean_mesh, decimate_mesh

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


class GaussianField:
    """The density field of a cloud, kept on the device so that it can be evaluated at arbitrary points afterwards.

    Builds what `extract_fields` builds, by the same kernels (one plan, one host wait; `.occ` has the same bits), and keeps
    the plan and the per-block lists alive.  Attributes: `.occ` (resolution,)*3, `.center` (3,), `.scale` (float),
    `.block_counts` (num_blocks,)*3 int32.  A model (anything with get_xyz, ...) has its `center` and `scale` set as
    `extract_fields` sets them."""

    def __init__(self, model_or_tensors, resolution: int = 128, num_blocks: int = 16, relax_ratio: float = 1.5):
        if num_blocks < 1:
            raise ValueError(f"GaussianField: num_blocks ({num_blocks}) must be at least 1")
        if resolution % num_blocks != 0:
            raise ValueError(f"GaussianField: resolution ({resolution}) must be a multiple of num_blocks ({num_blocks})")
        block_size = 2 / num_blocks
        (xyz, opacity, scaling, rotation), is_model = _model_tensors(model_or_tensors)
        _check_device((xyz, opacity, scaling, rotation), "GaussianField")
        dev = xyz.device
        self.resolution, self.num_blocks, self.num_gaussians = resolution, num_blocks, int(xyz.shape[0])
        self._state = None                                        # (info, axis, plan, lists) of a plan that lists something
        geo = None
        if xyz.shape[0] == 0:
            self.occ = torch.zeros([resolution] * 3, dtype=torch.float32, device=dev)
            self.block_counts = torch.zeros([num_blocks] * 3, dtype=torch.int32, device=dev)
        else:
            with torch.no_grad():
                axis = torch.linspace(-1, 1, resolution).to(dev)
                self.occ, self.block_counts, geo, sizes, plan, lists, info = _lib.load_binding().field_build(
                    xyz.detach(), opacity.detach().reshape(-1), scaling.detach(), rotation.detach(), axis, num_blocks,
                    block_size * relax_ratio, True)
            if sizes[0] == 0:
                geo = None
            if sizes[1] > 0:
                self._state = (info, axis, plan, lists)
        if geo is None:
            self.center, self.scale = torch.zeros(3, dtype=torch.float32, device=dev), 1.0
        else:
            self.center = torch.tensor(geo[:3], dtype=torch.float32, device=dev)
            self.scale = 1.8 / geo[3] if geo[3] > 0 else float("inf")
        if is_model:
            model_or_tensors.center, model_or_tensors.scale = self.center, self.scale

    def sample(self, points: torch.Tensor, colors: Optional[torch.Tensor] = None, normalized: bool = False):
        """(density (M,), normals (M,3), colors (M,3) or None) of the field at `points` (M,3), all fp32 on the device.

        `points` are world coordinates, or with normalized=True coordinates of the normalised cloud (the grid's
        linspace(-1, 1, resolution)), used untouched.  A point takes the list of the block its grid cell belongs to (a
        point on a grid sample: that sample's block, where the density equals `occ` bit for bit; a point outside the
        grid: the edge block).  normals: the unit vector from high density to low, -grad density / |grad density|, the
        side the faces of `marching_cubes` show; (0,0,0) where the gradient vanishes.  colors: the opacity-weighted mean
        sum(o e c) / sum(o e) of `colors` (P,3), one row per Gaussian of the cloud; (0,0,0) where the density is 0.
        Points with a NaN or infinite coordinate and points of a block that lists nothing return zeros.  A field that
        lists nothing, or M == 0: zeros without a launch.  Bit-reproducible, whatever the order of the points."""
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"GaussianField.sample: points must be (M, 3), got {tuple(points.shape)}")
        if colors is not None and (colors.dim() != 2 or colors.shape[0] != self.num_gaussians or colors.shape[1] != 3):
            raise ValueError(f"GaussianField.sample: colors must be ({self.num_gaussians}, 3), one row per Gaussian, got "
                             f"{tuple(colors.shape)}")
        _check_device((points,) if colors is None else (points, colors), "GaussianField.sample")
        M, dev = points.shape[0], points.device
        if self._state is None or M == 0:
            zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
            return zeros(M), zeros(M, 3), (None if colors is None else zeros(M, 3))
        with torch.no_grad():
            return _lib.load_binding().field_sample(*self._state, points.detach(),
                                                    None if colors is None else colors.detach(), bool(normalized))


SH_C0 = 0.28209479177387814


def gaussian_colors(model) -> torch.Tensor:
    """(P,3) the colour of every Gaussian as the rasterizer shows its degree-0 band: max(0, SH_C0 * _features_dc[:, 0] + 0.5).
    The higher SH bands depend on the view direction and are NOT baked: a mesh coloured with these shows the avatar's
    view-independent colour."""
    return torch.clamp_min(SH_C0 * model._features_dc.detach()[:, 0] + 0.5, 0.0)


def _finish_mesh(vertices, triangles, clean, decimate_target, min_f, min_d):
    """the reference's order: clean_mesh, then decimate_mesh when there are more triangles than the target"""
    if clean:
        vertices, triangles = clean_mesh(vertices, triangles, min_f=min_f, min_d=min_d)
    if decimate_target > 0 and triangles.shape[0] > decimate_target:
        vertices, triangles = decimate_mesh(vertices, triangles, decimate_target)
    return vertices, triangles


def extract_mesh(model, density_thresh: float = 1, resolution: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """(vertices (V,3) fp32 in world space, faces (T,3) int32) of the avatar's density iso-surface: the reference's
    extract_mesh up to (not including) clean_mesh / decimate_mesh.  `extract_clean_mesh` goes on from there."""
    if isinstance(model, (tuple, list)):
        occ, center, scale = extract_fields(model, resolution)
    else:
        occ = extract_fields(model, resolution)
        center, scale = model.center, model.scale
    vertices, triangles = marching_cubes(occ, density_thresh)
    vertices = vertices / (resolution - 1.0) * 2 - 1
    vertices = vertices / scale + center
    return vertices, triangles


def extract_clean_mesh(model, density_thresh: float = 1, resolution: int = 128, clean: bool = True, decimate_target: int = 0,
                       min_f: int = MIN_F, min_d: float = MIN_D) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's extract_mesh to its end, on the device: `extract_mesh`, then - in world space, in the reference's
    order - clean=True removes floaters, degenerate faces and unreferenced vertices (`meshclean.clean_mesh` with min_f,
    min_d) and decimate_target > 0 decimates to at most that many faces when the mesh has more
    (`meshclean.decimate_mesh`; the reference's decimate_target default is 1e5).  Not pymeshlab's algorithms
    (INTEGRATION.md 13).  clean=False, decimate_target=0 returns `extract_mesh`'s result, bit for bit."""
    vertices, triangles = extract_mesh(model, density_thresh, resolution)
    return _finish_mesh(vertices, triangles, clean, decimate_target, min_f, min_d)


def extract_mesh_attributes(model, density_thresh: float = 1, resolution: int = 128, colors: Optional[torch.Tensor] = None):
    """`extract_mesh` with vertex attributes (an extension; the reference stops at vertices and faces):
    (vertices, faces, normals (V,3), colors (V,3) or None).  vertices and faces are those of `extract_mesh`, bit for bit;
    normals and colors are the field's outward unit normal and opacity-weighted colour at every vertex
    (`GaussianField.sample` at the vertices' normalised coordinates, before they go to world space).  The Gaussians'
    colours are `colors` (P,3) if given; else `gaussian_colors(model)` for a model, and None for the four-tensor form.
    The raw iso-surface only: `extract_clean_mesh_attributes` is the same call for the cleaned, decimated mesh."""
    field = GaussianField(model, resolution)
    if colors is None and not isinstance(model, (tuple, list)):
        colors = gaussian_colors(model)
    vertices, triangles = marching_cubes(field.occ, density_thresh)
    vertices = vertices / (resolution - 1.0) * 2 - 1
    _, normals, vertex_colors = field.sample(vertices, colors, normalized=True)
    vertices = vertices / field.scale + field.center
    return vertices, triangles, normals, vertex_colors


def extract_clean_mesh_attributes(model, density_thresh: float = 1, resolution: int = 128, colors: Optional[torch.Tensor] = None,
                                  clean: bool = True, decimate_target: int = 0, min_f: int = MIN_F, min_d: float = MIN_D):
    """`extract_mesh_attributes` for the finished mesh: (vertices, faces, normals, colors or None) with vertices and faces
    those of `extract_clean_mesh(model, density_thresh, resolution, clean, decimate_target, min_f, min_d)`, bit for bit, and the
    normals and colours sampled at the FINAL vertices (`GaussianField.sample` in world coordinates, normalized=False) -
    a decimated vertex is a cell mean and lies beside the iso-surface, so its attributes are the field's there.  One
    field build serves the surface and the samples.  With clean=False and decimate_target=0 the mesh is the raw
    iso-surface (attributes sampled at its world-space vertices)."""
    field = GaussianField(model, resolution)
    if colors is None and not isinstance(model, (tuple, list)):
        colors = gaussian_colors(model)
    vertices, triangles = marching_cubes(field.occ, density_thresh)
    vertices = vertices / (resolution - 1.0) * 2 - 1
    vertices = vertices / field.scale + field.center
    vertices, triangles = _finish_mesh(vertices, triangles, clean, decimate_target, min_f, min_d)
    _, normals, vertex_colors = field.sample(vertices, colors, normalized=False)
    return vertices, triangles, normals, vertex_colors
