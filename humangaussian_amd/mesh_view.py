"""The mesh view: the posed body mesh (or an extracted, coloured mesh) drawn on the device by a forward-only HIP triangle
rasterizer (csrc/meshview.hip, include/hgs_rast.h: hgs_meshview_*).

Reference: animation.py
  :524-556   the display modes of the animation loop; `mesh` is the one this module serves
  :558-601   `render_mesh_normal`: clip = mvp . (v, 1), nvdiffrast's rasterize, three scatter_add_ of the face normals,
             nvdiffrast's interpolate, (n + 1) / 2 over a white background                     -> `MeshView.render_normals`

What is drawn is defined in include/hgs_rast.h (8 sub-pixel bits, an exact int64 coverage test with a top-left style
ownership rule, the nearest fragment with ties to the lower face index, perspective-correct u and v); tests/
mesh_view_reference.py restates it in numpy and the kernels match it bit for bit.  Differences from nvdiffrast: forward
only (no autograd, no antialias, no textures, no derivatives output); no near-plane clipping - a triangle with a vertex at
w <= 0 is dropped; both windings are drawn.  Nothing here has a CPU path: tensors on the CPU raise.

A rasterize or render call waits on the host once, for the 32-byte header that sizes the tiles' triangle lists (as the
density field and the mesh grid do).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

MAX_DIM = _lib.MESHVIEW_MAX_DIM
TILE = _lib.MESHVIEW_TILE
LIST_BATCH = _lib.MESHVIEW_LIST_BATCH          # triangles of a tile's list staged through LDS at a time
MAX_ATTR = _lib.MESHVIEW_MAX_ATTR


def _no_cpu(t):
    if isinstance(t, torch.Tensor) and t.device.type != "cuda":
        raise RuntimeError("humangaussian_amd: tensors must live on a HIP device (there is no CPU path)")


def mvp_from_camera(cam) -> torch.Tensor:
    """The (4, 4) matrix with clip = mvp . (v, 1) of a 3DGS camera: `cam.full_proj_transform` is applied to row vectors, so
    mvp is its transpose.  With it the mesh view and the Gaussian render of the same camera agree pixel for pixel: the
    sample of pixel (r, c) is the point the Gaussian rasterizer calls pixel (c, r)."""
    return cam.full_proj_transform.t().contiguous()


class MeshView:
    """faces (F, 3) integers, numpy or tensor; built once per topology: the vertex -> (face, corner) adjacency in CSR form
    (`adj_start` (V + 1,), `adj` (3 F,) = 3 face + corner, ascending inside a vertex).  One host read here (the range of the
    indices is checked)."""

    def __init__(self, faces, num_vertices: int, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("humangaussian_amd: a MeshView lives on a HIP device (there is no CPU path)")
        _no_cpu(faces)
        if not isinstance(faces, torch.Tensor):
            faces = torch.from_numpy(np.ascontiguousarray(np.asarray(faces).astype(np.int64)))
        if faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError(f"faces must be (F, 3), got {tuple(faces.shape)}")
        V = int(num_vertices)
        if V < 0:
            raise ValueError("num_vertices must not be negative")
        f = faces.detach().to(self.device, torch.int64)
        F = f.shape[0]
        if F > (1 << 24) - 1:
            raise ValueError("at most 2^24 - 1 faces (the face index travels in a float)")
        if F > 0 and (int(f.min()) < 0 or int(f.max()) >= V):
            raise ValueError(f"faces index vertices outside [0, {V})")
        self.num_vertices, self.num_faces = V, F
        self.faces = f.to(torch.int32).contiguous()
        flat = f.reshape(-1)
        order = torch.argsort(flat * max(3 * F, 1) + torch.arange(3 * F, device=self.device))
        self.adj = order.to(torch.int32).contiguous()
        start = torch.zeros(V + 1, dtype=torch.int64, device=self.device)
        if F > 0:
            start[1:] = torch.cumsum(torch.bincount(flat, minlength=V), 0)
        self.adj_start = start.to(torch.int32).contiguous()

    # ---- argument checks
    def _vertices(self, vertices) -> torch.Tensor:
        _no_cpu(vertices)
        if not isinstance(vertices, torch.Tensor):
            vertices = torch.from_numpy(np.ascontiguousarray(np.asarray(vertices, dtype=np.float32))).to(self.device)
        v = vertices.detach().to(self.device, torch.float32)
        if v.dim() == 2:
            v = v[None]
        if v.dim() != 3 or v.shape[1] != self.num_vertices or v.shape[2] != 3:
            raise ValueError(f"vertices must be ({self.num_vertices}, 3) or (B, {self.num_vertices}, 3), got {tuple(vertices.shape)}")
        return v.contiguous()

    def _mvp(self, mvp) -> torch.Tensor:
        _no_cpu(mvp)
        if not isinstance(mvp, torch.Tensor):
            mvp = torch.from_numpy(np.ascontiguousarray(np.asarray(mvp, dtype=np.float32))).to(self.device)
        m = mvp.detach().to(self.device, torch.float32)
        if m.dim() == 2:
            m = m[None]
        if m.dim() != 3 or tuple(m.shape[1:]) != (4, 4):
            raise ValueError(f"mvp must be (4, 4) or (B, 4, 4), got {tuple(mvp.shape)}")
        return m.contiguous()

    def _attr(self, attr) -> torch.Tensor:
        _no_cpu(attr)
        if not isinstance(attr, torch.Tensor):
            attr = torch.from_numpy(np.ascontiguousarray(np.asarray(attr, dtype=np.float32))).to(self.device)
        a = attr.detach().to(self.device, torch.float32)
        if a.dim() == 2:
            a = a[None]
        if a.dim() != 3 or a.shape[1] != self.num_vertices or not 1 <= a.shape[2] <= MAX_ATTR:
            raise ValueError(f"attr must be ({self.num_vertices}, C) or (B, {self.num_vertices}, C) with 1 <= C <= {MAX_ATTR}, "
                             f"got {tuple(attr.shape)}")
        return a.contiguous()

    @staticmethod
    def _size(H, W):
        H, W = int(H), int(W)
        if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
            raise ValueError(f"H and W must be in [1, {MAX_DIM}], got {H} x {W}")
        return H, W

    @staticmethod
    def _batch(B, t, what):
        if t.shape[0] not in (1, B):
            raise ValueError(f"{what} must hold one set for every view or one per view: {t.shape[0]} for {B} views")

    # ---- the calls
    @torch.no_grad()
    def vertex_normals(self, vertices) -> torch.Tensor:
        """vertices (V, 3) or (B, V, 3) -> unit normals (B, V, 3): the face normals cross(v1 - v0, v2 - v0) summed per vertex
        in the order of the adjacency (a gather, bit-reproducible), (0, 0, 1) where the sum vanishes."""
        v = self._vertices(vertices)
        return _lib.load_binding().meshview_normals(v, self.faces, self.adj_start, self.adj)

    @torch.no_grad()
    def rasterize(self, vertices, mvp, H: int, W: int, return_records: bool = False):
        """-> rast (B, H, W, 4) fp32 = (u, v, z, face + 1), zeros where nothing is drawn [, records (B, V, 4) int32: the
        vertex records the raster read]."""
        v, m = self._vertices(vertices), self._mvp(mvp)
        H, W = self._size(H, W)
        self._batch(m.shape[0], v, "vertices")
        rast, _, records = _lib.load_binding().meshview_draw(v, m, self.faces, H, W)
        return (rast, records) if return_records else rast

    @torch.no_grad()
    def interpolate(self, attr, rast) -> torch.Tensor:
        """attr (V, C) or (B, V, C), rast (B, H, W, 4) -> (B, H, W, C); zeros where rast has no face."""
        a = self._attr(attr)
        _no_cpu(rast)
        if not isinstance(rast, torch.Tensor) or rast.dim() != 4 or rast.shape[3] != 4:
            raise ValueError("rast must be a (B, H, W, 4) tensor")
        self._size(rast.shape[1], rast.shape[2])
        r = rast.detach().to(self.device, torch.float32).contiguous()
        self._batch(r.shape[0], a, "attr")
        return _lib.load_binding().meshview_interpolate(a, r, self.faces)

    @torch.no_grad()
    def render_normals(self, vertices, mvp, H: int, W: int, background: float = 1.0) -> torch.Tensor:
        """The reference's `render_mesh_normal`: (B, H, W, 3), (n + 1) / 2 of the interpolated, re-normalised vertex
        normals, `background` elsewhere.  Two launches for the normals and the vertex records aside, the image is shaded in
        the raster kernel: no rast is written."""
        v, m = self._vertices(vertices), self._mvp(mvp)
        H, W = self._size(H, W)
        self._batch(m.shape[0], v, "vertices")
        b = _lib.load_binding()
        normals = b.meshview_normals(v, self.faces, self.adj_start, self.adj)
        return b.meshview_draw(v, m, self.faces, H, W, normals, True, float(background), False)[1]

    @torch.no_grad()
    def render_attributes(self, vertices, attr, mvp, H: int, W: int, background: float = 0.0) -> torch.Tensor:
        """(B, H, W, C): the vertex attributes (the extracted mesh's colours, say) interpolated over the drawn faces,
        `background` elsewhere; bit-equal to `interpolate(attr, rasterize(...))` on the drawn pixels."""
        v, m, a = self._vertices(vertices), self._mvp(mvp), self._attr(attr)
        H, W = self._size(H, W)
        self._batch(m.shape[0], v, "vertices")
        self._batch(m.shape[0], a, "attr")
        return _lib.load_binding().meshview_draw(v, m, self.faces, H, W, a, False, float(background), False)[1]
