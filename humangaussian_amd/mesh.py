"""Closest point and signed distance of points to a triangle mesh on the GPU: the `cubvh.cuBVH` the reference builds once
per avatar to anchor its Gaussians on the body mesh (/root/reference/animation.py:333-378):

    BVH = cubvh.cuBVH(vertices, faces)
    mapping_dist, mapping_face, mapping_uvw = BVH.signed_distance(points, return_uvw=True, mode="raystab")

HIP kernels: csrc/mesh.hip through `hgs_mesh_grid_plan` / `hgs_mesh_grid_build` / `hgs_mesh_query` of the C ABI (a
uniform grid built once per mesh; `brute_force=True`: the O(P F) kernel over every face, the same results bit for bit).
The semantics - closest face with ties to the lowest index, Ericson barycentrics, the 64-ray stab that decides the sign -
are those of include/hgs_rast.h: cubvh's own sign test is modelled on instant-ngp's ray stab, whose exact directions this
module does not reproduce.  No CPU path: CPU tensors raise."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

MODES = ("raystab", "unsigned")


def _check_mode(mode: str) -> bool:
    """True for the signed mode; NotImplementedError for anything but the supported ones."""
    if mode not in MODES:
        raise NotImplementedError(f"signed_distance: mode {mode!r} is not supported; supported modes: {', '.join(MODES)}")
    return mode == "raystab"


def _on_device(x, dtype, device: Optional[torch.device], name: str) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        if x.device.type != "cuda":
            raise RuntimeError(f"humangaussian_amd: {name} must live on a HIP device (torch device type 'cuda'), got "
                               f"{x.device}; numpy arrays are uploaded, CPU tensors are not (there is no CPU path)")
        return x.to(device or x.device, dtype).contiguous()
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=device or "cuda").contiguous()


class MeshIndex:
    """A triangle mesh indexed for closest-point queries.  `vertices` (V,3) and `faces` (F,3): numpy arrays (uploaded to
    `device`, default the current HIP device) or HIP tensors.  The grid is built once, here; every query reuses it."""

    def __init__(self, vertices, faces, device=None):
        dev = torch.device(device) if device is not None else None
        if dev is not None and dev.type != "cuda":
            raise RuntimeError(f"humangaussian_amd: MeshIndex needs a HIP device (torch device type 'cuda'), got {dev}")
        self.vertices = _on_device(vertices, torch.float32, dev, "vertices")
        self.faces = _on_device(faces, torch.int32, self.vertices.device, "faces")
        if self.vertices.dim() != 2 or self.vertices.shape[1] != 3 or self.faces.dim() != 2 or self.faces.shape[1] != 3:
            raise ValueError(f"vertices must be (V, 3) and faces (F, 3), got {tuple(self.vertices.shape)} and "
                             f"{tuple(self.faces.shape)}")
        self.device = self.vertices.device
        self.grid, info = _lib.load_binding().mesh_build(self.vertices, self.faces)
        self.grid_dims, self.num_cells, self.num_refs = tuple(info[:3]), info[3], info[4]

    def _query(self, points, raystab: bool, return_uvw: bool, brute_force: bool):
        pts = _on_device(points, torch.float32, self.device, "points")
        if pts.shape[-1:] != (3,):
            raise ValueError(f"points must have shape (..., 3), got {tuple(pts.shape)}")
        lead = pts.shape[:-1]
        dist, face, uvw = _lib.load_binding().mesh_query(pts.reshape(-1, 3), self.vertices, self.faces,
                                                         None if brute_force else self.grid, raystab, return_uvw)
        return (dist.reshape(lead), face.to(torch.int64).reshape(lead),
                uvw.reshape(*lead, 3) if return_uvw else None)

    def unsigned_distance(self, positions, return_uvw: bool = False, brute_force: bool = False
                          ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """(dist >= 0 fp32, face int64, uvw fp32 (..., 3) or None) with the points' leading shape."""
        return self._query(positions, False, return_uvw, brute_force)

    def signed_distance(self, positions, return_uvw: bool = False, mode: str = "raystab", brute_force: bool = False
                        ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """As `unsigned_distance`, with dist negated for points inside the mesh (mode "raystab": all 64 rays of the fixed
        direction set hit a face).  mode "unsigned" skips the sign.  (cubvh's default mode, "watertight", is not
        provided: the reference always asks for "raystab".)"""
        return self._query(positions, _check_mode(mode), return_uvw, brute_force)
