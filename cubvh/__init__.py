"""Drop-in module name for the reference: `import cubvh; cubvh.cuBVH(vertices, faces).signed_distance(points,
return_uvw=True, mode="raystab")` (/root/reference/animation.py:333-340) resolves here when this repository is on sys.path;
implemented in HIP (humangaussian_amd/csrc/mesh.hip, `humangaussian_amd.mesh.MeshIndex`).  Only what the reference
calls: `signed_distance` ("raystab" and "unsigned" modes) and `unsigned_distance`."""
from humangaussian_amd.mesh import MeshIndex as cuBVH  # noqa: F401

__all__ = ["cuBVH"]
