"""CPU tests of the mesh queries (csrc/mesh.hip, humangaussian_amd/mesh.py, the `cubvh` shim): the fp64 reference
against closed-form answers and against the winding number, a numpy restatement of the grid plan and the shell search's
stop rule checked against the brute force, and the Python / C-ABI surface without a GPU.  The HIP kernels themselves run
in tests/test_gpu_mesh_anchor.py."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridfit_reference as G  # noqa: E402
import mesh_reference as R  # noqa: E402

F32 = np.float32

# ------------------------------------------------------------------------------------------------ the fp64 reference


def test_reference_closest_point_closed_forms():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    pts = np.array([[0.2, 0.3, 0.5],       # above the interior
                    [0.5, -0.4, 0.3],      # beyond edge v0-v1
                    [-1.0, -2.0, 0.0],     # beyond vertex v0
                    [1.0, 1.0, -1.0],      # beyond edge v1-v2
                    [0.0, 3.0, 0.0]])      # beyond vertex v2
    d2, face, uvw, _ = R.closest_point(pts, v, f)
    np.testing.assert_allclose(d2, [0.25, 0.16 + 0.09, 5.0, 0.5 + 1.0, 4.0], atol=1e-12)
    np.testing.assert_allclose(uvw, [[0.5, 0.2, 0.3], [0.5, 0.5, 0.0], [1, 0, 0], [0, 0.5, 0.5], [0, 0, 1]], atol=1e-12)
    assert (face == 0).all()
    # closest = u v0 + v v1 + w v2
    q = uvw @ v.astype(np.float64)
    np.testing.assert_allclose(((pts - q) ** 2).sum(1), d2, atol=1e-12)


def test_reference_cube_inside_outside_and_ties():
    v, f = R.cube(0.5)
    pts = np.array([[0.1, 0.2, -0.1], [0.0, 0.0, 0.0], [0.9, 0.0, 0.0], [0.0, -0.7, 0.6], [2.0, 2.0, 2.0]])
    d2, face, uvw, d2b = R.closest_point(pts, v, f)
    np.testing.assert_allclose(np.sqrt(d2), [0.3, 0.5, 0.4, np.hypot(0.2, 0.1), np.sqrt(3) * 1.5], atol=1e-12)
    assert list(R.raystab_inside(pts, v, f)) == [True, True, False, False, False]
    # the centre is 0.5 from all 12 faces: the lowest index wins, and the runner-up ties
    assert face[1] == 0 and d2b[1] == d2[1]
    assert np.allclose(uvw.sum(1), 1.0) and (uvw >= -1e-12).all()


@pytest.mark.parametrize("mesh", ["cube", "torus", "icosphere3"])
def test_reference_raystab_sign_equals_winding_sign_on_closed_meshes(mesh):
    v, f = {"cube": R.cube, "torus": R.torus, "icosphere3": lambda: R.icosphere(3)}[mesh]()
    assert R.signed_volume(v, f) > 0                      # outward winding
    rng = np.random.default_rng(1)
    pts = rng.uniform(-1.2, 1.2, (600, 3))
    wn = R.winding_number(pts, v, f)
    clear = np.abs(wn - np.round(wn)) < 1e-6               # (no point ON the surface)
    assert clear.mean() > 0.99
    inside = R.raystab_inside(pts, v, f)
    assert ((wn > 0.5) == inside)[clear].all()
    assert 0 < inside.sum() < len(pts)


def test_reference_skips_exactly_degenerate_faces():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3]], np.int32)        # face 0 is collinear: skipped
    assert list(R.valid_faces(v, f)) == [False, True]
    d2, face, _, _ = R.closest_point(np.array([[1.5, -0.1, 0.0]]), v, f)
    assert face[0] == 1 and np.isclose(d2[0], 0.25 + 0.01)


# ------------------------------------------------------------------------------------------------ grid restatement
# The plan (hgs_k_mesh_bbox / _grid_setup / _count_refs: the grid rule itself is gridfit_reference.py's) and the stop rule
# of mesh_grid_closest in numpy, fp32 where the device uses fp32.  The union of the cell lists of a block of cells = the
# faces whose bounding-box cells overlap the block, so a shell search is restated per face; after shell r the search stops
# when best d2 < reach^2 (margins as in mesh.hip).


def plan(v, f):
    v = v.astype(F32)
    fin = np.all(np.isfinite(v), axis=1)
    lo = v[fin].min(0)
    ext = (v[fin].max(0) - lo).astype(F32)
    nc_max = min(max(16 * len(f), 64), 1 << 22)
    lo, h, inv_h, g = G.grid(lo, ext, G.h0_mesh(ext, len(f)) if ext.max() > 0 else None, nc_max)
    ok = R.valid_faces(v, f)
    tri = v[f]                                             # (F, 3, 3)

    def cell(x):
        return G.cell1(x, lo, inv_h, g)
    c0, c1 = cell(tri.min(1)), cell(tri.max(1))
    refs = int(np.prod(c1 - c0 + 1, axis=1)[ok].sum())
    cmax = F32(np.max(np.abs(np.stack([lo, (lo + (g * h).astype(F32)).astype(F32)]))))
    return dict(lo=lo, h=h, inv_h=inv_h, g=g, ok=ok, c0=c0, c1=c1, refs=refs, cmax=cmax, cell=cell)


def grid_search(pts, v, f):
    """Per point: (d2 of the best face the grid search has seen when it stops, shells searched)."""
    G = plan(v, f)
    lo, h, g, ok, c0, c1 = G["lo"], G["h"], G["g"], G["ok"], G["c0"], G["c1"]
    v64 = v.astype(np.float64)
    a, b, c = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    out, shells = np.zeros(len(pts)), np.zeros(len(pts), np.int64)
    for i, p in enumerate(pts.astype(F32)):
        d2_all = R.closest_on_tris(p.astype(np.float64)[None], a, b, c)[0]
        d2_all[~ok] = np.inf
        cc = G["cell"](p[None])[0]
        rel = (p - lo).astype(F32)
        margin = F32(F32(1e-3) * h + F32(1e-5) * max(G["cmax"], F32(np.abs(p).max())))
        for r in range(int(g.max()) + 1):
            blo, bhi = np.maximum(cc - r, 0), np.minimum(cc + r, g - 1)
            seen = ok & np.all((c1 >= blo) & (c0 <= bhi), axis=1)
            best = d2_all[seen].min() if seen.any() else np.inf
            if np.all(blo == 0) and np.all(bhi == g - 1):
                break
            reach = F32(np.inf)
            for ax in range(3):
                if cc[ax] - r > 0:
                    reach = min(reach, F32(rel[ax] - F32(F32(cc[ax] - r) * h)))
                if cc[ax] + r < g[ax] - 1:
                    reach = min(reach, F32(F32(F32(cc[ax] + r + 1) * h) - rel[ax]))
            reach = F32(reach - margin)
            if reach > 0 and best < float(reach) * float(reach):
                break
        out[i], shells[i] = best, r
    return out, shells


def _surface(v, f, n, rng, off):
    v64 = v.astype(np.float64)
    k = rng.integers(0, len(f), n)
    r1, r2 = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 1, n)
    uvw = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], 1)
    p = np.einsum("ij,ijk->ik", uvw, v64[f[k]])
    return p + rng.uniform(-off, off, (n, 1)) * R.face_normals(v, f)[k]


def _huge_and_small():
    v, f = R.icosphere(3)
    big_v = np.array([[-6, -6, 0.3], [6, -6, 0.3], [0, 6, 0.3], [-6, 0.2, -6], [6, 0.2, -6], [0, 0.2, 6]], np.float32)
    return np.concatenate([v, big_v]), np.concatenate([f, np.array([[0, 1, 2], [3, 4, 5]], np.int32) + len(v)])


def _humanoid():
    from humangaussian_amd import synth
    return synth.humanoid_mesh()


CASES = {
    "surface_hugging": (lambda: R.icosphere(4), lambda v, f, rng: _surface(v, f, 150, rng, 1e-3)),
    "far_outliers": (lambda: R.torus(), lambda v, f, rng: rng.normal(size=(60, 3)) * 40.0),
    "outside_the_box": (lambda: R.cube(), lambda v, f, rng: rng.uniform(-3, 3, (200, 3))),
    "huge_among_small": (_huge_and_small, lambda v, f, rng: np.concatenate([rng.uniform(-1.5, 1.5, (150, 3)),
                                                                            _surface(v, f[:-2], 50, rng, 0.05)])),
    "translated_far": (lambda: tuple(x + np.float32(1000.0) if x.dtype == np.float32 else x for x in R.torus()),
                       lambda v, f, rng: np.concatenate([_surface(v, f, 100, rng, 0.02), 1000.0 + rng.uniform(-1, 1, (100, 3))])),
    "humanoid_open": (_humanoid, lambda v, f, rng: np.concatenate([_surface(v, f, 100, rng, 0.03), rng.uniform(-0.8, 0.8, (100, 3))])),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_grid_stop_rule_never_stops_before_the_closest_face(case):
    make_mesh, make_pts = CASES[case]
    v, f = make_mesh()
    rng = np.random.default_rng(7)
    pts = make_pts(v, f, rng).astype(np.float32)
    got, shells = grid_search(pts, v, f)
    want = R.closest_point(pts, v, f)[0]
    np.testing.assert_array_equal(got, want)               # the true closest face was among the faces searched
    G = plan(v, f)
    assert G["refs"] >= G["ok"].sum() and np.prod(G["g"]) <= max(16 * len(f), 64)
    if case == "surface_hugging":                           # and the search stays local where it should
        assert np.median(shells) <= 2, np.bincount(shells)


def test_plan_grid_of_the_icosphere():
    v, f = R.icosphere(5)
    assert len(f) == 20480
    G = plan(v, f)
    occupied = np.zeros(np.prod(G["g"]), np.int64)
    for (x0, y0, z0), (x1, y1, z1) in zip(G["c0"], G["c1"]):
        for z in range(z0, z1 + 1):
            for y in range(y0, y1 + 1):
                occupied[(z * G["g"][1] + y) * G["g"][0] + x0:(z * G["g"][1] + y) * G["g"][0] + x1 + 1] += 1
    per_cell = occupied[occupied > 0]
    assert 1.0 <= per_cell.mean() <= 8.0, per_cell.mean()    # ~1-4 faces per occupied cell
    assert G["refs"] == occupied.sum()


# ------------------------------------------------------------------------------------------------ import and errors


def test_cubvh_resolves_to_the_shim_with_the_reference_keywords():
    import cubvh
    from humangaussian_amd.mesh import MeshIndex
    assert cubvh.cuBVH is MeshIndex
    assert os.path.dirname(os.path.abspath(cubvh.__file__)).endswith("cubvh")
    sig = inspect.signature(MeshIndex.signed_distance)
    assert {"positions", "return_uvw", "mode", "brute_force"} <= set(sig.parameters)
    assert {"positions", "return_uvw", "brute_force"} <= set(inspect.signature(MeshIndex.unsigned_distance).parameters)
    assert list(inspect.signature(MeshIndex).parameters)[:2] == ["vertices", "faces"]
    from humangaussian_amd.animation import AvatarAnimator, anchor_to_mesh
    assert list(inspect.signature(anchor_to_mesh).parameters) == ["points", "vertices", "faces", "max_error"]
    assert "max_error" in inspect.signature(AvatarAnimator.from_rest_pose).parameters


def test_unsupported_mode_raises_not_implemented():
    from humangaussian_amd.mesh import MeshIndex
    idx = object.__new__(MeshIndex)                         # the mode is checked before anything touches a device
    for mode in ("watertight", "RAYSTAB", ""):
        with pytest.raises(NotImplementedError, match="raystab, unsigned"):
            idx.signed_distance(torch.zeros(4, 3), return_uvw=True, mode=mode)


def test_cpu_tensors_raise():
    from humangaussian_amd.animation import anchor_to_mesh
    from humangaussian_amd.mesh import MeshIndex
    v, f = R.cube()
    with pytest.raises(RuntimeError, match="HIP device"):
        MeshIndex(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(RuntimeError, match="HIP device"):
        MeshIndex(v, f, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        anchor_to_mesh(torch.zeros(5, 3), v, f)


class MeshGridInfo(ctypes.Structure):
    """ctypes mirror of hgs_mesh_grid_info (include/hgs_rast.h)."""
    _fields_ = [("bmin", ctypes.c_uint32 * 3), ("bmax", ctypes.c_uint32 * 3), ("dims", ctypes.c_int32 * 3),
                ("ncells", ctypes.c_uint32), ("origin", ctypes.c_float * 3), ("cell", ctypes.c_float),
                ("num_faces", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("num_refs", ctypes.c_uint64)]


def test_c_abi_sizing_and_argument_errors_without_gpu():
    from humangaussian_amd import _lib
    _lib.build()
    lib = _lib.load()
    assert ctypes.sizeof(MeshGridInfo) == 72 and MeshGridInfo.num_refs.offset == 64
    info = MeshGridInfo()
    info.dims[:] = [10, 20, 30]
    info.ncells, info.cell, info.num_faces, info.num_refs = 6000, 0.1, 1000, 5000
    n = lib.hgs_mesh_grid_bytes(ctypes.byref(info))
    assert n >= 1000 * 48 + 6001 * 4 + 6000 * 4 + 5000 * 4 and n % 256 == 0
    info.num_refs = 6000
    al = lambda x: -(-x // 256) * 256  # noqa: E731
    assert lib.hgs_mesh_grid_bytes(ctypes.byref(info)) == n - al(5000 * 4) + al(6000 * 4)     # 4 bytes per reference
    assert lib.hgs_mesh_grid_bytes(None) == 0
    info.ncells = 6001                                                    # not the product of the dims: not a plan
    assert lib.hgs_mesh_grid_bytes(ctypes.byref(info)) == 0
    info.ncells, info.num_refs = 6000, 1 << 31                            # too many references
    assert lib.hgs_mesh_grid_bytes(ctypes.byref(info)) == 0
    # (P, points, V, vertices, F, faces, grid, mode, dist, face, uvw, stream)
    assert lib.hgs_mesh_query(0, None, 0, None, 0, None, None, 1, None, None, None, None) == 0     # P = 0: nothing to do
    assert lib.hgs_mesh_query(-1, None, 0, None, 0, None, None, 1, None, None, None, None) == -1
    assert lib.hgs_mesh_query(5, None, 3, None, 0, None, None, 1, None, None, None, None) == -1    # F = 0 with P > 0
    assert lib.hgs_mesh_query(0, None, 0, None, 1, None, None, 2, None, None, None, None) == -1    # unknown mode
    assert lib.hgs_mesh_grid_plan(3, None, 0, None, None, None) == -1
    assert lib.hgs_mesh_grid_build(3, None, 1, None, ctypes.byref(info), None, None) == -1
    assert lib.hgs_abi_version() == 17
