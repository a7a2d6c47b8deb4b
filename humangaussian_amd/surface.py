"""The first stage of a run on the device: area-uniform samples of the body surface and the initial Gaussians built from them.

Reference (paths in the HumanGaussian tree):
  threestudio/utils/poser.py:225-231                `Skeleton.sample_smplx_points(N)`: trimesh.sample.sample_surface on the
                                                    CPU                                    -> `SurfaceSampler.sample`,
                                                                                              `sample_surface`
  threestudio/systems/GaussianDreamer.py:220-232    `pcb()`: the samples as a BasicPointCloud of constant colour 0.5
  gaussiansplatting/scene/gaussian_model.py:124-147 `GaussianModel.create_from_pcd`: two uploads, distCUDA2, some fifteen
                                                    small torch kernels                    -> `create_from_points`,
                                                                                              `create_from_pcd`

HIP kernels: csrc/surface.hip through `hgs_surface_cdf` / `hgs_surface_sample` / `hgs_init_gaussians` of the C ABI; the
definition (fp64 table of face areas, Philox4x32-10 per sample index, integer barycentric coordinates) is
include/hgs_rast.h's.  trimesh draws from numpy's generator: these are OTHER samples of the same distribution.

Beyond the reference: every sample knows its face and barycentric coordinates, so the cloud is born anchored on the body
(`SurfaceSampler.anchors`, `init_from_body` -> `animation.MeshAnchoredGaussians`) and needs no closest-point query.
No CPU path: CPU tensors raise."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .mesh import _on_device


def _check_mesh_shapes(vertices, faces) -> None:
    vs, fs = tuple(np.shape(vertices)), tuple(np.shape(faces))
    if len(vs) != 2 or vs[1] != 3 or len(fs) != 2 or fs[1] != 3:
        raise ValueError(f"vertices must be (V, 3) and faces (F, 3), got {vs} and {fs}")
    if fs[0] == 0:
        raise ValueError("the mesh has no faces: there is no surface to sample")
    if fs[0] > _lib.SURFACE_MAX_FACES:
        raise ValueError(f"at most {_lib.SURFACE_MAX_FACES} faces, got {fs[0]}")


def _check_draw(n, seed, offset) -> None:
    if int(n) != n or n < 0:
        raise ValueError(f"n must be a non-negative integer, got {n!r}")
    for name, x in (("seed", seed), ("offset", offset)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < 1 << 64:
            raise ValueError(f"{name} must be an integer in [0, 2^64), got {x!r}")


class SurfaceSampler:
    """A triangle mesh prepared for area-uniform sampling.  `vertices` (V,3) and `faces` (F,3): numpy arrays (uploaded to
    `device`, default the current HIP device) or HIP tensors.  The fp64 table of face areas is built once, here (the one
    host wait: its total and the number of faces a sample can fall on are read back); every `sample` is one launch.
    Faces of area 0, of a non-finite area or with a vertex index outside [0, V) are never sampled."""

    def __init__(self, vertices, faces, device=None):
        _check_mesh_shapes(vertices, faces)
        dev = torch.device(device) if device is not None else None
        if dev is not None and dev.type != "cuda":
            raise RuntimeError(f"humangaussian_amd: SurfaceSampler needs a HIP device (torch device type 'cuda'), got {dev}")
        self.vertices = _on_device(vertices, torch.float32, dev, "vertices")
        self.faces = _on_device(faces, torch.int32, self.vertices.device, "faces")
        self.device = self.vertices.device
        self.num_faces = int(self.faces.shape[0])
        self._table, self.area, self.num_sampled_faces = _lib.load_binding().surface_build(self.vertices, self.faces)
        if not self.area > 0.0:
            raise ValueError(f"no face of the mesh has a positive area (total {self.area}): there is no surface to sample")

    @property
    def cdf(self) -> torch.Tensor:
        """(F,) fp64: entry f = the area of faces 0 .. f, the table a sample's face is looked up in"""
        return self._table[1:]

    def sample(self, n: int, seed: int = 0, offset: int = 0, return_anchors: bool = False):
        """n points (n,3) fp32, or (points, face (n,) int32, uvw (n,3) fp32) as the kernel wrote them (int32 is what
        `MeshAnchoredGaussians` keeps).  Sample i depends on (seed, offset + i) alone: rows k .. k+m of a call are the rows
        of `sample(m, seed, offset=offset + k)`, bit for bit."""
        _check_draw(n, seed, offset)
        pts, face, uvw = _lib.load_binding().surface_sample(self.vertices, self.faces, self._table, int(n), int(seed),
                                                            int(offset), bool(return_anchors))
        return (pts, face, uvw) if return_anchors else pts

    def anchors(self, face, uvw):
        """The samples as Gaussians anchored on this mesh (distance 0 along the face normal): `.positions(vertices)` of a
        posed mesh moves them with it; at this mesh it gives the samples' own bits."""
        from .animation import MeshAnchoredGaussians
        face = torch.as_tensor(face)
        return MeshAnchoredGaussians(self.faces, face, uvw, torch.zeros(face.shape, dtype=torch.float32), device=self.device)


def sample_surface(vertices, faces, n: int, seed: int = 0):
    """`trimesh.sample.sample_surface(mesh, n)` for the reference's call site: (samples (n,3) fp32, face_index (n,) int64),
    on the device."""
    _check_draw(n, seed, 0)
    pts, face, _ = SurfaceSampler(vertices, faces).sample(n, seed=seed, return_anchors=True)
    return pts, face.to(torch.int64)


_NAMES = ("features_dc", "features_rest", "scaling", "rotation", "opacity", "max_radii2D")


def create_from_points(points, colors=None, max_sh_degree: int = 0) -> dict:
    """The tensors `create_from_pcd` builds from a cloud, as a dict: xyz (P,3) (the points themselves), features_dc (P,1,3),
    features_rest (P,(D+1)^2-1,3), scaling (P,3), rotation (P,4), opacity (P,1), max_radii2D (P,).  `points` (P,3) and
    `colors` (P,3, in [0,1]; None: the constant 0.5 of the reference's pcb()) are HIP tensors.  One distCUDA2 and one launch."""
    if not 0 <= int(max_sh_degree) <= 63:
        raise ValueError(f"max_sh_degree must be in 0 .. 63, got {max_sh_degree}")
    pts = torch.as_tensor(points)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be (P, 3), got {tuple(pts.shape)}")
    if colors is not None and tuple(np.shape(colors)) != tuple(pts.shape):
        raise ValueError(f"colors must be {tuple(pts.shape)} like the points, got {tuple(np.shape(colors))}")
    pts = _on_device(pts.detach(), torch.float32, None, "points")
    col = None if colors is None else _on_device(torch.as_tensor(colors).detach(), torch.float32, pts.device, "colors")
    b = _lib.load_binding()
    out = b.init_gaussians(b.knn_mean_dist2(pts, False), col, (int(max_sh_degree) + 1) ** 2)
    return dict(zip(("xyz",) + _NAMES, [pts] + list(out)))


def create_from_pcd(model, pcd_or_points, spatial_lr_scale: float, colors=None):
    """`GaussianModel.create_from_pcd(pcd, spatial_lr_scale)` applied to `model`: the reference's GaussianModel or any object
    with its attributes (`max_sh_degree` is read).  `pcd_or_points`: an object with `.points` / `.colors` (numpy arrays or
    tensors: the reference's BasicPointCloud) or a (P,3) HIP tensor / numpy array, then with `colors` (None: 0.5).  Sets
    `spatial_lr_scale`, the six nn.Parameters `_xyz`, `_features_dc`, `_features_rest`, `_scaling`, `_rotation`, `_opacity`
    (requires_grad, contiguous, the reference's shapes) and `max_radii2D`.  Returns `model`."""
    if hasattr(pcd_or_points, "points"):
        points, colors = pcd_or_points.points, getattr(pcd_or_points, "colors", None) if colors is None else colors
    else:
        points = pcd_or_points
    if not isinstance(points, torch.Tensor):
        points = torch.as_tensor(np.asarray(points), dtype=torch.float32, device="cuda")
    if colors is not None and not isinstance(colors, torch.Tensor):
        colors = torch.as_tensor(np.asarray(colors), dtype=torch.float32, device=points.device)
    t = create_from_points(points, colors, int(getattr(model, "max_sh_degree", 0)))
    model.spatial_lr_scale = spatial_lr_scale
    xyz = t["xyz"].clone() if t["xyz"].data_ptr() == points.data_ptr() else t["xyz"]      # the model owns its points
    model._xyz = torch.nn.Parameter(xyz.requires_grad_(True))
    for name in _NAMES[:-1]:
        setattr(model, "_" + name, torch.nn.Parameter(t[name].requires_grad_(True)))
    model.max_radii2D = t["max_radii2D"]
    return model


def init_from_body(model, vertices, faces, n: int, seed: int = 0, spatial_lr_scale: float = 1.0):
    """`pcb()` + `create_from_pcd` from a body mesh on the device: n area-uniform samples of (vertices, faces) become the
    model's initial Gaussians (colour 0.5).  Returns the `MeshAnchoredGaussians` of the new cloud: row i of `_xyz` is
    `anchors.positions(vertices)[i]`, bit for bit, and follows any posed mesh of the same faces."""
    sampler = SurfaceSampler(vertices, faces)
    pts, face, uvw = sampler.sample(n, seed=seed, return_anchors=True)
    create_from_pcd(model, pts, spatial_lr_scale)
    return sampler.anchors(face, uvw)
