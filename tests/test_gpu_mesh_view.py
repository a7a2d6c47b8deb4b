"""GPU tests of the mesh view (humangaussian_amd/mesh_view.py, csrc/meshview.hip; include/hgs_rast.h: hgs_meshview_*)
against the numpy restatement tests/mesh_view_reference.py: the raster bit for bit on the kernel's own vertex records, the
vertex records and the vertex normals against float64 within a gate built from the float32 restatement's own error, the
hand-built edge cases, the list-length boundaries of the LDS staging, batch and order invariance, the raw C ABI behind guard
zones, and the animator's mesh frame against its Gaussian frame."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mesh_view_reference as R
from humangaussian_amd import _lib, mesh_view
from humangaussian_amd.mesh_view import MeshView

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SHAPES = [(64, 64), (52, 75), (97, 130)]
EPS32 = float(np.finfo(np.float32).eps)
EYE = np.eye(4, dtype=np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_REF = {}


def _ref_rast(rec, faces, H, W):
    """the reference raster of one view's records - computed once per distinct input, shared by the tests, never changed"""
    key = (rec.tobytes(), np.asarray(faces).tobytes(), H, W)
    if key not in _REF:
        r = R.rasterize_records(rec, faces, H, W)
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _assert_rast(rast, records, faces, H, W):
    """ids equal, u, v and z bit-equal, for every view"""
    rast, records = rast.cpu().numpy(), records.cpu().numpy()
    assert rast.shape == (len(records), H, W, 4)
    for b in range(len(records)):
        want = _ref_rast(records[b], faces, H, W)
        assert np.array_equal(rast[b, ..., 3], want[..., 3]), (b, int((rast[b, ..., 3] != want[..., 3]).sum()))
        assert np.array_equal(_bits(rast[b, ..., :3]), _bits(want[..., :3])), b
    return rast


def _draw_and_check(vertices, faces, mvp, H, W, records_exact=True):
    """rasterize one hand-built view, hold it to the reference, return (rast (H, W, 4), records (V, 4)) as numpy"""
    view = MeshView(faces, len(vertices), device=DEV)
    rast, rec = view.rasterize(_dev(vertices), _dev(mvp), H, W, return_records=True)
    if records_exact:
        assert np.array_equal(rec[0].cpu().numpy(), R.vertex_records(vertices, mvp, H, W))
    return _assert_rast(rast, rec, faces, H, W)[0], rec[0].cpu().numpy()


def _tri_px(points, size=32, z=0.5):
    """vertices of points (x, y[, z]) given in pixel coordinates of a size x size image (mvp = identity)"""
    return np.asarray([(R.ndc_of_pixel(p[0], size), R.ndc_of_pixel(p[1], size), p[2] if len(p) > 2 else z) for p in points],
                      np.float32)


def _soup_mvps(B):
    m = np.stack([EYE, EYE, EYE]).copy()
    m[1, 0, 0], m[1, 1, 1], m[1, 0, 3] = 0.8, 0.9, 0.11
    m[2, 0, 0], m[2, 1, 1], m[2, 1, 3], m[2, 3, 3] = 1.3, 1.2, -0.07, 1.25
    return m[:B]


# ------------------------------------------------------------------------------------------------- 1. raster exactness

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("scene", ["humanoid", "soup"])
def test_raster_and_shading_equal_the_reference_on_the_kernels_own_records(scene, shape, B):
    H, W = shape
    if scene == "humanoid":
        v, f, mvps, _ = R.humanoid_views(H, W)
        mvps = mvps[:B]
    else:
        v, f = R.triangle_soup(300, seed=5)
        mvps = _soup_mvps(B)
    view = MeshView(f, len(v), device=DEV)
    vd, md = _dev(v), _dev(mvps)
    rast_d, rec_d = view.rasterize(vd, md, H, W, return_records=True)
    rast = _assert_rast(rast_d, rec_d, f, H, W)
    hit = rast[..., 3] > 0
    if scene == "humanoid":
        assert hit.any() and not hit.all()
    else:                                      # the screen-sized triangles cover the image; many small ones lie in front
        assert hit.any() and len(np.unique(rast[..., 3])) > 50
    # interpolate: one attribute set for all views (C = 5) and one per view (C = 8)
    rng = np.random.default_rng(11)
    shared, per_view = rng.standard_normal((len(v), 5)).astype(np.float32), rng.standard_normal((B, len(v), 8)).astype(np.float32)
    got = view.interpolate(_dev(shared), rast_d).cpu().numpy()
    got_b = view.interpolate(_dev(per_view), rast_d).cpu().numpy()
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(R.interpolate(shared, rast[b], f))), b
        assert np.array_equal(_bits(got_b[b]), _bits(R.interpolate(per_view[b], rast[b], f))), b
    # the fused images: bit-equal to rasterize followed by interpolate, and to the reference's stage 6
    fused = view.render_attributes(vd, _dev(per_view), md, H, W, background=0.25).cpu().numpy()
    assert np.array_equal(_bits(fused), _bits(np.where(hit[..., None], got_b, np.float32(0.25))))
    normals = view.vertex_normals(vd)
    nimg = view.render_normals(vd, md, H, W).cpu().numpy()
    two_step = view.interpolate(normals, rast_d).cpu().numpy()
    n_host = normals[0].cpu().numpy()
    for b in range(B):
        assert np.array_equal(_bits(fused[b]), _bits(R.shade_attributes(per_view[b], rast[b], f, 0.25))), b
        assert np.array_equal(_bits(nimg[b]), _bits(R.shade_normals(n_host, rast[b], f, 1.0))), b
        assert np.array_equal(_bits(two_step[b]), _bits(R.interpolate(n_host, rast[b], f))), b
    assert (nimg[~hit] == 1.0).all() and np.isfinite(nimg).all() and nimg.min() >= 0.0 and nimg.max() <= 1.0


# --------------------------------------------------------------------------------------- 2. / 3. against float64

_RATIOS = {}


def _record_ratios(case_id, entry):
    _RATIOS[case_id] = entry
    if not os.environ.get("HGS_WRITE_PROFILES"):
        return
    doc = {"what": "per case of tests/test_gpu_mesh_view.py: records_* = max |x_fix - xs64|, |y_fix - ys64| of hgs_meshview_plan "
                   "(fixed-point units, the 0.5 of the rounding included), the float32 restatement's own error and the gate "
                   "0.5 + max(4 ref, 16 eps32 (max(H, W) << 8)); normals_* = max |n - n64| of hgs_meshview_normals, the "
                   "float32 restatement's error and the gate max(4 ref, 16 eps32), in units of eps32",
           "device": torch.cuda.get_device_name(0), "cases": dict(sorted(_RATIOS.items()))}
    with open(os.path.join(ROOT, "profiles", "mesh_view_parity.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_vertex_records_against_fp64(shape):
    H, W = shape
    v, f, mvps, _ = R.humanoid_views(H, W)
    _, rec = MeshView(f, len(v), device=DEV).rasterize(_dev(v), _dev(mvps), H, W, return_records=True)
    rec = rec.cpu().numpy()
    err = ref = 0.0
    differ = 0
    for b, m in enumerate(mvps):
        xs64, ys64, zw64, c3 = R.vertex_stage64(v, m, H, W)
        xs32, ys32, zw32, iw32, valid = R.vertex_stage32(v, m, H, W)
        assert valid.all() and (rec[b, :, 0] != R.INVALID).all()
        err = max(err, np.abs(rec[b, :, 0] - xs64).max(), np.abs(rec[b, :, 1] - ys64).max())
        ref = max(ref, np.abs(xs32.astype(np.float64) - xs64).max(), np.abs(ys32.astype(np.float64) - ys64).max())
        differ += int((rec[b, :, 0] != np.rint(xs64)).sum() + (rec[b, :, 1] != np.rint(ys64)).sum())
        # depth and 1 / w travel as float32 bits: within a few ulp of the float64 values
        assert np.abs(rec[b, :, 2].copy().view(np.float32) - zw64).max() <= 16 * EPS32 * np.abs(zw64).max()
        assert np.abs(rec[b, :, 3].copy().view(np.float32) * c3 - 1).max() <= 16 * EPS32
    gate = max(4.0 * ref, 16.0 * EPS32 * (max(H, W) << 8))
    entry = {"records_err": err, "records_ref": ref, "records_gate": 0.5 + gate, "records_off_fp64_rounding": differ}
    print(shape, entry)
    _record_ratios(f"records_{H}x{W}", entry)
    assert err <= 0.5 + gate, entry


def _normals_mesh():
    """the humanoid with three extra vertices: one without faces, and one whose two faces cancel"""
    from humangaussian_amd import synth
    v, f = synth.humanoid_mesh()
    n = len(v)
    extra = np.array([[2, 2, 2], [3, 0, 0], [3, 1, 0], [4, 0, 1]], np.float32)
    v = np.concatenate([v, extra])
    f = np.concatenate([f, np.array([[n + 1, n + 2, n + 3], [n + 1, n + 3, n + 2]], np.int32)])
    return v, f, n


def test_vertex_normals_against_fp64():
    v, f, n0 = _normals_mesh()
    view = MeshView(f, len(v), device=DEV)
    assert np.array_equal(view.adj_start.cpu().numpy(), R.csr_adjacency(f, len(v))[0])
    assert np.array_equal(view.adj.cpu().numpy(), R.csr_adjacency(f, len(v))[1])
    moved = (v * np.float32(1.1) + np.float32(0.05)).astype(np.float32)
    got = view.vertex_normals(_dev(np.stack([v, moved]))).cpu().numpy()
    assert got.shape == (2, len(v), 3)
    assert np.array_equal(_bits(view.vertex_normals(_dev(v)).cpu().numpy()[0]), _bits(got[0]))
    for b, verts in enumerate((v, moved)):
        assert (got[b, n0:] == np.array([0, 0, 1], np.float32)).all()            # no faces; faces that cancel
        n32, n64 = R.vertex_normals(verts, f), R.vertex_normals(verts, f, np.float64)
        body = slice(0, n0)
        err, ref = np.abs(got[b, body] - n64[body]).max(), np.abs(n32[body].astype(np.float64) - n64[body]).max()
        gate = max(4.0 * ref, 16.0 * EPS32)
        entry = {"normals_err_over_eps": err / EPS32, "normals_ref_over_eps": ref / EPS32, "normals_gate_over_eps": gate / EPS32,
                 "normals_off_fp32_restatement": int((_bits(got[b]) != _bits(n32)).any(1).sum())}
        print(b, entry)
        _record_ratios(f"normals_{b}", entry)
        assert err <= gate, entry


# ------------------------------------------------------------------------------------------------- 4. hand-built cases

def test_single_triangle_in_both_windings():
    v = _tri_px([(3.3, 2.1), (27.9, 9.4), (11.2, 29.7)])
    a, _ = _draw_and_check(v, np.array([[0, 1, 2]], np.int32), EYE, 32, 32)
    b, _ = _draw_and_check(v, np.array([[0, 2, 1]], np.int32), EYE, 32, 32)
    c, _ = _draw_and_check(v, np.array([[1, 2, 0]], np.int32), EYE, 32, 32)
    assert (a[..., 3] > 0).sum() > 150
    assert np.array_equal(a[..., 3], b[..., 3]) and np.array_equal(a[..., 3], c[..., 3])
    # (the depth is the same up to the rounding of three weights that sum to one in another order)
    assert np.abs(a[..., 2] - b[..., 2]).max() <= 4 * EPS32 and np.abs(a[..., 2] - c[..., 2]).max() <= 4 * EPS32


def test_shared_edge_quad_on_pixel_centres():
    v = _tri_px([(4.5, 4.5), (20.5, 4.5), (20.5, 20.5), (4.5, 20.5)])
    for faces in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [0, 2, 3]], [[1, 2, 3], [3, 0, 1]]):
        rast, _ = _draw_and_check(v, np.asarray(faces, np.int32), EYE, 32, 32)
        hit = rast[..., 3] > 0
        want = np.zeros((32, 32), bool)
        want[4:20, 5:21] = True                   # the top row and the right column are the quad's; every sample once
        assert np.array_equal(hit, want)
        assert set(np.unique(rast[..., 3])) == {0.0, 1.0, 2.0}


def test_coincident_triangles_at_equal_depth_go_to_the_lower_id():
    tri = [(3.3, 2.1), (27.9, 9.4), (11.2, 29.7)]
    v = _tri_px(tri + tri, z=0.0)                 # depth 0 at every corner: z = 0 exactly whatever the corner order
    for faces in ([[0, 1, 2], [3, 4, 5]], [[3, 4, 5], [0, 1, 2]], [[0, 1, 2], [5, 4, 3]]):
        rast, _ = _draw_and_check(v, np.asarray(faces, np.int32), EYE, 32, 32)
        assert set(np.unique(rast[..., 3])) == {0.0, 1.0}


def test_interpenetrating_triangles():
    v = _tri_px([(2, 2, 0.1), (30, 3, 0.9), (15, 30, 0.5), (30, 2, 0.1), (2, 3, 0.9), (16, 30, 0.5)])
    rast, _ = _draw_and_check(v, np.array([[0, 1, 2], [3, 4, 5]], np.int32), EYE, 32, 32)
    assert (rast[..., 3] == 1).sum() > 50 and (rast[..., 3] == 2).sum() > 50


def test_zero_area_triangle_draws_nothing_and_its_neighbour_everything():
    v = _tri_px([(2, 2), (16, 16), (30, 30), (2, 2), (30, 4), (16, 28)])
    rast, _ = _draw_and_check(v, np.array([[0, 1, 2], [3, 4, 5], [3, 3, 4]], np.int32), EYE, 32, 32)
    assert set(np.unique(rast[..., 3])) == {0.0, 2.0}


def test_triangle_with_a_vertex_behind_or_not_a_number_is_dropped():
    # w = z: the vertices at z = -1 and z = 0 have c3 <= 0
    mvp = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.5, 0], [0, 0, 1, 0]], np.float32)
    good = [(-0.8, -0.8, 1.0), (0.8, -0.7, 1.0), (0.0, 0.8, 1.0)]
    v = np.asarray(good + [(-0.5, 0.5, -1.0), (0.5, 0.5, 0.0), (np.nan, 0.0, 1.0), (0.9, 0.9, 1.0)], np.float32)
    faces = np.array([[0, 1, 3], [0, 1, 2], [1, 2, 4], [2, 0, 5], [1, 6, 2]], np.int32)
    rast, rec = _draw_and_check(v, faces, mvp, 32, 32)
    assert (rec[3:6, 0] == R.INVALID).all() and (rec[3:6, 1:] == 0).all() and (rec[[0, 1, 2, 6], 0] != R.INVALID).all()
    assert set(np.unique(rast[..., 3])) == {0.0, 2.0, 5.0} and (rast[..., 3] == 2).sum() > 100 and (rast[..., 3] == 5).sum() > 20


def test_guard_band():
    # W = 64: |xs| < 2^23 is |x_ndc 0.5 + 0.5| < 512.  8 screens out (x_ndc = +-16) is far inside; 1100 is beyond
    inside = np.asarray([(-16.0, -0.5, 0.5), (0.9, -0.9, 0.5), (0.9, 0.9, 0.5), (16.0, 0.3, 0.3), (-0.9, 0.8, 0.3), (-0.9, -0.2, 0.3),
                         (1100.0, 0.0, 0.5), (0.0, -0.9, 0.5), (0.0, 0.9, 0.5), (0.5, -1022.9, 0.4), (-0.5, 0.9, 0.4), (0.6, 0.9, 0.4)],
                        np.float32)
    faces = np.arange(12, dtype=np.int32).reshape(4, 3)
    rast, rec = _draw_and_check(inside, faces, EYE, 64, 64)
    assert rec[6, 0] == R.INVALID and (np.delete(rec[:, 0], 6) != R.INVALID).all()
    assert abs(int(rec[9, 1])) > 2 ** 22
    ids = set(np.unique(rast[..., 3]))
    assert ids == {0.0, 1.0, 2.0, 4.0}


def test_depth_range_is_applied_per_fragment():
    v = _tri_px([(1, 1, -2.0), (31, 1, 2.0), (16, 31, 0.0)])
    rast, _ = _draw_and_check(v, np.array([[0, 1, 2]], np.int32), EYE, 32, 32)
    hit = rast[..., 3] > 0
    assert hit.sum() > 100 and rast[hit][:, 2].min() >= -1.0 and rast[hit][:, 2].max() <= 1.0
    # the triangle's own footprint is wider: columns near both ends are cut off
    assert not hit[2, 2:6].any() and not hit[2, 27:30].any() and hit[2, 14:18].all()


def test_triangle_entirely_off_screen():
    v = np.asarray([(2.0, 0.0, 0.5), (3.0, 0.0, 0.5), (2.5, 1.0, 0.5), (-0.5, -3.0, 0.5), (0.5, -2.0, 0.5), (0.0, -1.5, 0.5)], np.float32)
    view = MeshView(np.array([[0, 1, 2], [3, 4, 5]], np.int32), 6, device=DEV)
    rast = view.rasterize(_dev(v), _dev(EYE), 52, 75)
    assert rast.shape == (1, 52, 75, 4) and not rast.any()
    img = view.render_normals(_dev(v), _dev(EYE), 52, 75, background=0.5)
    assert img.shape == (1, 52, 75, 3) and (img == 0.5).all()


# --------------------------------------------------------------------------------------------------- 5. list boundaries

@pytest.mark.parametrize("nearest", ["first", "middle", "last"])
@pytest.mark.parametrize("n", [mesh_view.LIST_BATCH - 1, mesh_view.LIST_BATCH, mesh_view.LIST_BATCH + 1, 2 * mesh_view.LIST_BATCH + 1])
def test_list_length_boundaries(n, nearest):
    v, f, near = R.stacked_quads(n, nearest)
    rast, rec = _draw_and_check(v, f, EYE, 32, 32)
    assert R.tile_list_lengths(rec, f, 32, 32).tolist() == [[0, 0], [0, n]]
    assert rast[20, 27, 3] == 2 * near + 1 and rast[20, 27, 2] == np.float32(0.25)
    assert (rast[..., 3] > 0).sum() == 13 * 13


# -------------------------------------------------------------------------------------------------------- 6. invariance

def test_batch_views_repeats_and_face_order():
    H, W = 97, 130
    v, f, mvps, _ = R.humanoid_views(H, W)
    view = MeshView(f, len(v), device=DEV)
    vd, md = _dev(v), _dev(mvps)
    rast, rec = view.rasterize(vd, md, H, W, return_records=True)
    nimg = view.render_normals(vd, md, H, W)
    again, rec2 = view.rasterize(vd, md, H, W, return_records=True)
    assert torch.equal(rast.view(torch.int32), again.view(torch.int32)) and torch.equal(rec, rec2)
    assert torch.equal(nimg.view(torch.int32), view.render_normals(vd, md, H, W).view(torch.int32))
    for b in range(3):
        one, rec1 = view.rasterize(vd, md[b:b + 1], H, W, return_records=True)
        assert torch.equal(one[0].view(torch.int32), rast[b].view(torch.int32)) and torch.equal(rec1[0], rec[b])
        assert torch.equal(view.render_normals(vd, md[b], H, W)[0].view(torch.int32), nimg[b].view(torch.int32))
    # one mesh per view: the same mesh three times is the shared mesh
    stacked = view.rasterize(vd[None].repeat(3, 1, 1), md, H, W)
    assert torch.equal(stacked.view(torch.int32), rast.view(torch.int32))
    # a permutation of the faces permutes the ids and changes nothing else
    perm = np.random.default_rng(3).permutation(len(f))
    prast = MeshView(f[perm], len(v), device=DEV).rasterize(vd, md, H, W).cpu().numpy()
    rast = rast.cpu().numpy()
    hit = rast[..., 3] > 0
    assert np.array_equal(prast[..., 3] > 0, hit)
    assert np.array_equal(perm[prast[..., 3][hit].astype(np.int64) - 1], rast[..., 3][hit].astype(np.int64) - 1)
    assert np.array_equal(_bits(prast[..., :3]), _bits(rast[..., :3]))


# ----------------------------------------------------------------------------------------------------------- 7. raw ABI

def test_raw_abi_calls_leave_the_guard_zones_intact_and_write_every_byte():
    H, W, B, C = 52, 75, 3, 3
    lib = _lib.load()
    v, f, mvps, _ = R.humanoid_views(H, W)
    V, F = len(v), len(f)
    adj_start, adj = R.csr_adjacency(f, V)
    vd, fd, md, sd, ad = _dev(v), _dev(f), _dev(mvps), _dev(adj_start), _dev(adj)
    GUARD = 4096
    sizes = {"records": B * V * 16, "plan": lib.hgs_meshview_plan_bytes(B, F, H, W), "info": 32, "rast": B * H * W * 16,
             "image": B * H * W * C * 4, "normals": V * 12, "image2": B * H * W * C * 4}
    assert sizes["plan"] > 0
    bufs = {k: torch.full((GUARD + n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV) for k, n in sizes.items()}
    ptr = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    a = _lib.HgsMeshviewArgs()
    a.B, a.V, a.F, a.H, a.W, a.C, a.shade_normals, a.background = B, V, F, H, W, C, 1, 1.0
    a.vertex_stride, a.attr_stride = 0, 0
    a.vertices, a.mvp, a.faces, a.adj_start, a.adj = vd.data_ptr(), md.data_ptr(), fd.data_ptr(), sd.data_ptr(), ad.data_ptr()
    a.records, a.plan, a.info, a.normals = ptr["records"], ptr["plan"], ptr["info"], ptr["normals"]
    assert lib.hgs_meshview_normals(ctypes.byref(a), sp) == 0
    assert lib.hgs_meshview_plan(ctypes.byref(a), sp) == 0
    stream.synchronize()
    info = _lib.HgsMeshviewInfo.from_buffer_copy(bufs["info"][GUARD:GUARD + 32].cpu().numpy().tobytes())
    assert (info.B, info.V, info.F, info.H, info.W) == (B, V, F, H, W) and info.num_refs > 0
    sizes["lists"] = lib.hgs_meshview_list_bytes(ctypes.byref(info))
    assert sizes["lists"] >= 4 * info.num_refs
    bufs["lists"] = torch.full((GUARD + sizes["lists"] + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    a.lists = bufs["lists"].data_ptr() + GUARD
    a.attr, a.rast, a.image = ptr["normals"], ptr["rast"], ptr["image"]
    assert lib.hgs_meshview_draw(ctypes.byref(a), ctypes.byref(info), sp) == 0
    a.rast_in, a.image, a.shade_normals = ptr["rast"], ptr["image2"], 0
    assert lib.hgs_meshview_interpolate(ctypes.byref(a), sp) == 0
    stream.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, n in sizes.items():
        assert (host[k][:GUARD] == 0xFF).all() and (host[k][GUARD + n:] == 0xFF).all(), k

    def out(k, dtype, shape):
        return np.frombuffer(host[k][GUARD:GUARD + sizes[k]].tobytes(), dtype).reshape(shape)
    records, rast = out("records", np.int32, (B, V, 4)), out("rast", np.float32, (B, H, W, 4))
    image, image2, normals = out("image", np.float32, (B, H, W, C)), out("image2", np.float32, (B, H, W, C)), out("normals", np.float32, (V, 3))
    # 0xFFFFFFFF is a NaN and, as an integer, -1: no valid record, raster value, colour or normal looks like it
    assert not np.isnan(rast).any() and not np.isnan(image).any() and not np.isnan(image2).any() and not np.isnan(normals).any()
    assert (records != -1).all()
    lists = np.frombuffer(host["lists"][GUARD:GUARD + 4 * info.num_refs].tobytes(), np.uint32)
    assert (lists < F).all()                                               # every list entry was written
    n32 = R.vertex_normals(v, f)
    assert np.abs(normals - n32).max() <= 16 * EPS32
    for b in range(B):
        want = _ref_rast(records[b], f, H, W)
        assert np.array_equal(_bits(rast[b]), _bits(want))
        assert np.array_equal(_bits(image[b]), _bits(R.shade_normals(normals, want, f, 1.0)))
        assert np.array_equal(_bits(image2[b]), _bits(R.interpolate(normals, want, f)))
        assert info.num_refs >= R.tile_list_lengths(records[b], f, H, W).sum()
    assert info.num_refs == sum(R.tile_list_lengths(records[b], f, H, W).sum() for b in range(B))


# -------------------------------------------------------------------------------------------------------- 8. end to end

class _Cloud:
    """The reference GaussianModel's six tensors and getters for a dense, opaque, isotropic cloud."""
    active_sh_degree = max_sh_degree = 0

    def __init__(self, xyz):
        P = len(xyz)
        self._xyz = torch.as_tensor(xyz, device=DEV)
        self._features_dc, self._features_rest = torch.zeros(P, 1, 3, device=DEV), torch.zeros(P, 0, 3, device=DEV)
        op = float(np.log(R.CLOUD_OPACITY / (1 - R.CLOUD_OPACITY)))
        self._opacity = torch.full((P, 1), op, device=DEV)
        self._scaling = torch.full((P, 3), float(np.log(R.CLOUD_SCALE)), device=DEV)
        self._rotation = torch.tensor([[1.0, 0, 0, 0]], device=DEV).repeat(P, 1)

    get_xyz = property(lambda m: m._xyz)
    get_features = property(lambda m: torch.cat((m._features_dc, m._features_rest), dim=1))
    get_opacity = property(lambda m: torch.sigmoid(m._opacity))
    get_scaling = property(lambda m: torch.exp(m._scaling))
    get_rotation = property(lambda m: torch.nn.functional.normalize(m._rotation))


def test_animator_mesh_frame_matches_its_gaussian_frame():
    """`AvatarAnimator.render_mesh_frame` and `render_frame` through one camera (frame 0 of the reference's orbit: radius 2,
    fovy 50, 96 x 96): the mesh's silhouette against alpha > 0.5 of 12 000 opaque Gaussians of scale 0.01 sampled on the
    same mesh.  On the CPU - the numpy raster against the oracle's alpha of the same cloud - the two agree on 96.93 % of the
    pixels (the cloud is about half a pixel fatter all round: 11.0 % of the pixels against the mesh's 7.9 %); the kernels
    are held to that share minus 2 points."""
    from humangaussian_amd import synth
    from humangaussian_amd.animation import AvatarAnimator, orbit_frame_camera
    H = W = 96
    v, f = synth.humanoid_mesh()
    anim = AvatarAnimator.from_rest_pose(_Cloud(R.surface_cloud(v, f)), v, f, white_background=True, device=DEV)
    assert int(anim.keep.sum()) >= 11990
    cam = orbit_frame_camera(0, H, W, device=DEV)
    mesh = anim.render_mesh_frame(_dev(v), cam)
    assert mesh.shape == (H, W, 3) and mesh.device.type == "cuda" and not mesh.requires_grad
    view = anim._mesh_view
    rast = view.rasterize(_dev(v), mesh_view.mvp_from_camera(cam), H, W)[0]
    sil = rast[..., 3] > 0
    assert (mesh[~sil] == 1.0).all() and 0.05 < float(sil.float().mean()) < 0.12
    assert torch.equal(mesh.view(torch.int32), view.render_normals(_dev(v), mesh_view.mvp_from_camera(cam), H, W)[0].view(torch.int32))
    anim.gaussians._xyz = anim.anchors.positions(_dev(v))
    alpha = anim.renderer.render(cam)["alpha"]
    share = float(((alpha.reshape(H, W) > 0.5) == sil).float().mean())
    print("silhouette agreement", share)
    assert share >= 0.9693 - 0.02, share
    assert anim.render_mesh_frame(_dev(v), cam) is not None and anim._mesh_view is view          # built once


# ------------------------------------------------------------------------------------------------------------ 9. errors

def test_interface_errors_and_empty_inputs():
    v, f = R.triangle_soup(4, seed=1)
    view = MeshView(f, len(v), device=DEV)
    vd, md = _dev(v), _dev(EYE)
    with pytest.raises(RuntimeError, match="HIP device"):
        view.rasterize(torch.from_numpy(v), md, 16, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        view.rasterize(vd, torch.from_numpy(EYE), 16, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        view.vertex_normals(torch.from_numpy(v))
    with pytest.raises(RuntimeError, match="HIP device"):
        view.interpolate(torch.zeros(len(v), 3), torch.zeros(1, 4, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        MeshView(f, len(v), device="cpu")
    for H, W in ((0, 16), (16, 0), (4097, 16), (16, 4097)):
        with pytest.raises(ValueError):
            view.rasterize(vd, md, H, W)
        with pytest.raises(ValueError):
            view.render_normals(vd, md, H, W)
    with pytest.raises(ValueError):
        view.rasterize(vd[:-1], md, 16, 16)
    with pytest.raises(ValueError):
        view.rasterize(vd, md[0, :3], 16, 16)
    with pytest.raises(ValueError):
        view.rasterize(vd[None].repeat(2, 1, 1), md[None].repeat(3, 1, 1), 16, 16)
    with pytest.raises(ValueError):
        view.interpolate(torch.zeros(len(v), 9, device=DEV), torch.zeros(1, 4, 4, 4, device=DEV))
    with pytest.raises(ValueError):
        view.interpolate(torch.zeros(len(v), 3, device=DEV), torch.zeros(1, 4, 4, 3, device=DEV))
    with pytest.raises(ValueError):
        view.render_attributes(vd, torch.zeros(2, len(v), 3, device=DEV), md, 16, 16)
    with pytest.raises(ValueError):
        MeshView(np.array([[0, 1, 12]]), 12, device=DEV)
    with pytest.raises(ValueError):
        MeshView(np.zeros((2, 4), np.int32), 12, device=DEV)
    # B = 0 and F = 0: empty or background results
    none = md[None][:0]
    assert view.rasterize(vd, none, 16, 20).shape == (0, 16, 20, 4)
    assert view.render_normals(vd, none, 16, 20).shape == (0, 16, 20, 3)
    empty = MeshView(np.zeros((0, 3), np.int32), len(v), device=DEV)
    rast, rec = empty.rasterize(vd, md, 16, 20, return_records=True)
    assert rast.shape == (1, 16, 20, 4) and not rast.any()
    assert np.array_equal(rec[0].cpu().numpy(), R.vertex_records(v, EYE, 16, 20))
    assert (empty.render_normals(vd, md, 16, 20, background=0.75) == 0.75).all()
    assert (empty.vertex_normals(vd) == torch.tensor([0.0, 0.0, 1.0], device=DEV)).all()
    assert not empty.interpolate(torch.ones(len(v), 2, device=DEV), rast).any()
