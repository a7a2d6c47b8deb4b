"""CPU tests of the mesh view (include/hgs_rast.h: hgs_meshview_*): they keep the numpy restatement and the inputs of
tests/test_gpu_mesh_view.py honest - the coverage rule is watertight, the sampled views show enough of the mesh, the
list-boundary scenes have the lengths they are named after, and `mvp_from_camera` lands on the Gaussian rasterizer's pixels.
No kernel runs here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_view_reference as R
from humangaussian_amd import _lib, mesh_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_and_exports_the_mesh_view():
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(hgs_meshview_\w+)\s*\(", hdr, flags=re.M))
    assert declared == {"hgs_meshview_plan_bytes", "hgs_meshview_normals", "hgs_meshview_plan", "hgs_meshview_list_bytes",
                        "hgs_meshview_draw", "hgs_meshview_interpolate"}
    assert declared <= set(_lib.EXPORTS)
    for name, value in (("MAX_DIM", 4096), ("TILE", 16), ("LIST_BATCH", 256), ("MAX_ATTR", 8)):
        assert int(re.search(rf"#define HGS_MESHVIEW_{name}\s+(\d+)", hdr).group(1)) == value == getattr(_lib, "MESHVIEW_" + name)
    assert mesh_view.LIST_BATCH == _lib.MESHVIEW_LIST_BATCH
    assert ctypes.sizeof(_lib.HgsMeshviewInfo) == 32
    a = _lib.HgsMeshviewArgs
    assert a.vertex_stride.offset == 32 and a.vertices.offset == 48 and ctypes.sizeof(a) == 48 + 14 * 8


def test_sizing_and_argument_validation_without_gpu():
    _lib.build()
    lib = _lib.load()
    assert lib.hgs_meshview_plan_bytes(1, 100, 64, 64) > 0 and lib.hgs_meshview_plan_bytes(1, 100, 64, 64) % 256 == 0
    assert lib.hgs_meshview_plan_bytes(1, 100, 0, 64) == 0 and lib.hgs_meshview_plan_bytes(1, 100, 64, 4097) == 0
    assert lib.hgs_meshview_plan_bytes(-1, 100, 64, 64) == 0 and lib.hgs_meshview_plan_bytes(65536, 1, 64, 64) == 0
    info = _lib.HgsMeshviewInfo(num_refs=1000)
    assert lib.hgs_meshview_list_bytes(ctypes.byref(info)) == 4096
    info.num_refs = 1 << 31
    assert lib.hgs_meshview_list_bytes(ctypes.byref(info)) == ctypes.c_size_t(-1).value
    a = _lib.HgsMeshviewArgs(B=1, V=3, F=1, H=0, W=16)
    for fn in (lib.hgs_meshview_plan, lib.hgs_meshview_interpolate):
        assert fn(ctypes.byref(a), None) == -1
    a.H = 16
    assert lib.hgs_meshview_plan(ctypes.byref(a), None) == -1          # NULL pointers with B > 0
    assert lib.hgs_meshview_draw(ctypes.byref(a), ctypes.byref(info), None) == -1
    a.B = 0
    for fn in (lib.hgs_meshview_plan, lib.hgs_meshview_normals, lib.hgs_meshview_interpolate):
        assert fn(ctypes.byref(a), None) == 0                            # B == 0: nothing to do
    assert lib.hgs_meshview_plan(None, None) == -1


def test_cpu_tensors_and_bad_shapes_raise():
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh_view.MeshView(np.zeros((1, 3), np.int32), 3, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh_view.MeshView(torch.zeros(1, 3, dtype=torch.int32), 3)


def grid_mesh(n=6, seed=0):
    """an n x n quad grid with every vertex on a pixel centre (pixels 2 .. 2 + n): per quad a random diagonal, and per
    triangle a random winding and corner rotation"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(((n + 1) ** 2, 4), np.int32)
    for r in range(n + 1):
        for c in range(n + 1):
            rec[r * (n + 1) + c] = ((c + 2) * 256 + 128, (r + 2) * 256 + 128, np.float32(0.5).view(np.int32), np.float32(1).view(np.int32))
    faces = []
    for r in range(n):
        for c in range(n):
            i00, i01, i10, i11 = r * (n + 1) + c, r * (n + 1) + c + 1, (r + 1) * (n + 1) + c, (r + 1) * (n + 1) + c + 1
            tris = [(i00, i01, i11), (i00, i11, i10)] if rng.integers(2) else [(i00, i01, i10), (i01, i11, i10)]
            for t in tris:
                t = list(t)
                if rng.integers(2):
                    t = t[::-1]
                k = int(rng.integers(3))
                faces.append(t[k:] + t[:k])
    return rec, np.asarray(faces, np.int32)


def test_coverage_is_watertight():
    n = 6
    for seed in range(4):
        rec, faces = grid_mesh(n, seed)
        rast, counts = R.rasterize_records(rec, faces, 12, 12, return_counts=True)
        # every sample strictly inside the grid - on vertices, on shared edges, on diagonals - is covered exactly once
        assert (counts[3:2 + n, 3:2 + n] == 1).all(), counts
        assert set(np.unique(counts)) <= {0, 1}
        # the grid spans samples 2 .. 2 + n.  With u x v = u_x v_y - u_y v_x and rows growing with y the rule gives a
        # horizontal edge to the triangle below it and a vertical edge to the triangle on its left: the grid owns its top
        # row and its right column, and nobody owns its bottom row and its left column
        want = np.zeros_like(counts)
        want[2:2 + n, 3:2 + n + 1] = 1
        assert np.array_equal(counts, want), counts
        assert counts.sum() == n * n
        assert ((rast[..., 3] > 0) == (counts > 0)).all()


@pytest.mark.parametrize("H,W", [(64, 64), (52, 75), (97, 130)])
def test_sampled_views_meet_their_quotas(H, W):
    v, f, mvps, _ = R.humanoid_views(H, W)
    assert v.shape == (2304, 3) and f.shape == (4320, 3)
    for m in mvps:
        rec = R.vertex_records(v, m, H, W)
        assert (rec[:, 0] != R.INVALID).all()
        rast = R.rasterize_records(rec, f, H, W)
        hit = rast[..., 3] > 0
        assert hit.mean() >= 0.05, hit.mean()
        assert len(np.unique(rast[..., 3][hit])) >= 200
        z = rast[..., 2][hit]
        assert z.min() > 0.0 and z.max() < 1.0


def test_list_boundary_scenes_have_their_lengths():
    B = mesh_view.LIST_BATCH
    for n in (B - 1, B, B + 1, 2 * B + 1):
        for nearest in ("first", "middle", "last"):
            v, f, near = R.stacked_quads(n, nearest)
            assert len(f) == n
            rec = R.vertex_records(v, np.eye(4, dtype=np.float32), 32, 32)
            lengths = R.tile_list_lengths(rec, f, 32, 32)
            assert lengths.tolist() == [[0, 0], [0, n]]
            rast = R.rasterize_records(rec, f, 32, 32)
            # (row 20, column 27) lies in the first triangle of every layer, also of a last layer that is a lone triangle
            assert rast[20, 27, 3] == 2 * near + 1 and rast[20, 27, 2] == np.float32(0.25)
            assert (rast[17:30, 17:30, 3] > 0).all() and (rast[..., 3] > 0).sum() == 13 * 13


def test_mvp_from_camera_lands_on_the_gaussian_rasterizers_pixels():
    from humangaussian_amd import synth
    H, W = 97, 130
    v, _ = synth.humanoid_mesh()
    for az in (0.0, 30.0, 200.0):
        cam = synth.orbit_camera(10.0, az, 1.6, 50.0, H, W)
        mvp = mesh_view.mvp_from_camera(cam).numpy()
        assert np.array_equal(mvp, cam.full_proj_transform.numpy().T)
        xs, ys, _, _ = R.vertex_stage64(v, mvp, H, W)
        # the Gaussian rasterizer: p_view = (v, 1) . world_view_transform, pix = f x / z + W / 2 - 0.5
        pv = np.concatenate([v.astype(np.float64), np.ones((len(v), 1))], 1) @ cam.world_view_transform.numpy().astype(np.float64)
        fx, fy = W / (2.0 * math.tan(cam.FoVx / 2.0)), H / (2.0 * math.tan(cam.FoVy / 2.0))
        px, py = fx * pv[:, 0] / pv[:, 2] + W / 2.0 - 0.5, fy * pv[:, 1] / pv[:, 2] + H / 2.0 - 0.5
        # (the matrices are stored in float32: 1e-5 pixels is their rounding, not the convention's)
        assert np.abs(xs / 256.0 - 0.5 - px).max() < 1e-4 and np.abs(ys / 256.0 - 0.5 - py).max() < 1e-4


def test_fp32_vertex_stage_stays_close_to_fp64():
    """the figures the GPU test's gate is built from: the float32 restatement's own error, in fixed-point units"""
    H, W = 97, 130
    v, _, mvps, _ = R.humanoid_views(H, W)
    for m in mvps:
        xs, ys, _, _, valid = R.vertex_stage32(v, m, H, W)
        xs64, ys64, _, _ = R.vertex_stage64(v, m, H, W)
        assert valid.all()
        err = max(np.abs(xs - xs64).max(), np.abs(ys - ys64).max())
        assert err < 16 * np.finfo(np.float32).eps * (max(H, W) << 8)


def test_vertex_normals_restatement():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1], [1, 2, 4]], np.int32)          # vertex 0: two faces that cancel; vertex 3: no face
    n = R.vertex_normals(v, f)
    assert np.array_equal(n[0], [0, 0, 1]) and np.array_equal(n[3], [0, 0, 1])
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    start, adj = R.csr_adjacency(f, 5)
    assert start.tolist() == [0, 2, 5, 8, 8, 9] and adj[:2].tolist() == [0, 3]
