"""What follows marching cubes in the reference's `extract_mesh` (gs_renderer.py:333-361), on the GPU:
the floaters of the iso-surface removed by connected components, the mesh decimated to a face budget.

The reference calls kiui's `clean_mesh(vertices, triangles, remesh=True, remesh_size=0.015)` and
`decimate_mesh(vertices, triangles, decimate_target)`, pymeshlab on the CPU.  pymeshlab's algorithms are NOT reproduced:
no isotropic remeshing, no quadric edge collapse (the decimation is vertex clustering on a uniform grid: parallel,
order-independent, exactly specified), no non-manifold repair, no texture coordinates, no "keep only the largest
component".  HIP kernels: csrc/meshclean.hip through `hgs_meshclean_*` of the C ABI; include/hgs_rast.h states the
semantics in full, tests/mesh_clean_reference.py restates them in numpy.  Every result is the same
bits from call to call and for every order of the face list.  No CPU path: CPU tensors raise."""
from __future__ import annotations

import torch

from . import _lib

# [UPSTREAM-KNOWLEDGE] kiui.mesh_utils.clean_mesh's defaults (min_f=64, min_d=20, the percentages pymeshlab's
# "remove isolated pieces" filters take), as far as known: kiui is not available where this was written.
MIN_F = 64
MIN_D = 20.0


def _inputs(vertices, faces, what):
    for t in (vertices, faces):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"humangaussian_amd: {what} needs tensors on a HIP device (torch device type 'cuda'), got "
                               f"{getattr(t, 'device', type(t))}; there is no CPU path")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices must be (V, 3), got {tuple(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be (F, 3), got {tuple(faces.shape)}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: faces must be int32 or int64, got {faces.dtype}")
    if vertices.shape[0] > _lib.MESHCLEAN_MAX_ITEMS or faces.shape[0] > _lib.MESHCLEAN_MAX_ITEMS:
        raise ValueError(f"{what}: at most 2^29 vertices and faces")
    vertices = vertices.detach().to(torch.float32).contiguous()
    faces = faces.detach()
    if faces.dtype == torch.int64:
        if faces.numel() and (int(faces.min()) < -2 ** 31 or int(faces.max()) >= 2 ** 31):
            raise ValueError(f"{what}: faces hold values outside the int32 range")
        faces = faces.to(torch.int32)
    return vertices, faces.contiguous()


def _bad_faces(what, count, V):
    if count:
        raise ValueError(f"{what}: {count} faces index vertices outside [0, {V})")


def mesh_components(vertices: torch.Tensor, faces: torch.Tensor, return_rounds: bool = False):
    """(labels (V,) int32, comp_faces (V,) int32, comp_diag2 (V,) fp32) of a mesh on the device.

    labels[v] is the smallest vertex index of v's component (vertices are connected through the faces that share them; a
    vertex no face references is a component of its own).  Per component, at its label and 0 elsewhere: the number of
    its faces and the squared diagonal of its bounding box in fp32.  A face with an index outside [0, V) raises
    ValueError with the count.  return_rounds appends the number of label-propagation rounds the call took.
    V == 0 or F == 0 launches nothing."""
    vertices, faces = _inputs(vertices, faces, "mesh_components")
    V, dev = vertices.shape[0], vertices.device
    if V == 0 or faces.shape[0] == 0:
        out = (torch.arange(V, dtype=torch.int32, device=dev), torch.zeros(V, dtype=torch.int32, device=dev),
               torch.zeros(V, dtype=torch.float32, device=dev))
        return out + (0,) if return_rounds else out
    labels, comp_faces, comp_diag2, rounds, bad = _lib.load_binding().meshclean_components(vertices, faces)
    _bad_faces("mesh_components", bad, V)
    out = (labels, comp_faces, comp_diag2)
    return out + (rounds,) if return_rounds else out


def clean_mesh(vertices: torch.Tensor, faces: torch.Tensor, min_f: int = MIN_F, min_d: float = MIN_D,
               return_index: bool = False):
    """(vertices (V',3) fp32, faces (F',3) int32) without floaters, degenerate faces and unreferenced vertices.

    A face is kept iff its three indices are distinct, its component has at least `min_f` faces and its component's
    bounding-box diagonal is at least `min_d` percent of the whole mesh's (compared squared, in fp32: the header spells
    the operations).  A vertex is kept iff a kept face references it.  Kept vertices come in ascending original index,
    kept faces in original order, re-indexed.  return_index appends vertex_src (V',) int32, the kept vertices' original
    indices.  What kiui's clean_mesh does beyond that - merging close vertices, repairing non-manifold edges, isotropic
    remeshing - is out of scope.  A face with an index outside [0, V) raises.  V == 0 or F == 0 launches nothing."""
    vertices, faces = _inputs(vertices, faces, "clean_mesh")
    V, dev = vertices.shape[0], vertices.device
    if V == 0 or faces.shape[0] == 0:
        out = (vertices.new_zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32, device=dev))
        return out + (torch.zeros(0, dtype=torch.int32, device=dev),) if return_index else out
    try:
        v, f, src, _ = _lib.load_binding().meshclean_clean(vertices, faces, int(min_f), float(min_d), bool(return_index))
    except RuntimeError as e:
        if "faces index vertices outside" in str(e):
            raise ValueError(str(e)) from None
        raise
    return (v, f, src) if return_index else (v, f)


def decimate_mesh(vertices: torch.Tensor, faces: torch.Tensor, target: int, return_info: bool = False):
    """(vertices (V',3) fp32, faces (F',3) int32) with at most `target` faces, by vertex clustering.

    The vertices are binned into cubic cells of edge emax / g from the mesh's box minimum (emax: the longest extent,
    1 <= g <= 1024); g is the result of a fixed bisection over the number of faces whose three vertices lie in three
    different cells, so the budget is never exceeded.  One new vertex per cell that such a face references, at the mean
    of ALL input vertices in the cell (accumulated in integers on a fixed lattice: order-independent), ordered by the
    cell's smallest member index; the faces in original order, orientation kept, of duplicates (the same vertex set in
    any order) the lowest index.  No quadric placement, no texture coordinates.
    target <= 0 or F <= target: the input comes back bit for bit (the reference's `if`); a mesh without extent comes
    back without faces.  return_info appends {"grid": g, "cell": h, "input_faces": F, "probe_launches": n} (None for the
    no-op cases)."""
    vertices, faces = _inputs(vertices, faces, "decimate_mesh")
    F = faces.shape[0]
    target = int(target)
    if target <= 0 or F <= target:
        return (vertices, faces, None) if return_info else (vertices, faces)
    try:
        v, f, g, h, launches = _lib.load_binding().meshclean_decimate(vertices, faces, target)
    except RuntimeError as e:
        if "faces index vertices outside" in str(e):
            raise ValueError(str(e)) from None
        raise
    if return_info:
        return v, f, {"grid": int(g), "cell": float(h), "input_faces": F, "probe_launches": int(launches)}
    return v, f
