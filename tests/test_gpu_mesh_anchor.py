"""GPU tests of the mesh queries (csrc/mesh.hip through humangaussian_amd.mesh / the `cubvh` shim) and of the anchoring
built on them (animation.anchor_to_mesh, AvatarAnimator.from_rest_pose): the grid against the brute-force kernel bit for
bit, both against the fp64 reference (tests/mesh_reference.py), the sign on closed meshes, the reference's own call and
rebuild (/root/reference/animation.py:333-371), and a 500k-point query on the 20,480-face icosphere."""
import math
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _humanoid():
    from humangaussian_amd import synth
    return synth.humanoid_mesh()


MESHES = {"icosphere5": lambda: R.icosphere(5), "cube": R.cube, "torus": R.torus, "humanoid": _humanoid}
CLOSED = ("icosphere5", "cube", "torus")


def _surface(v, f, n, rng, off, bary_min=0.0):
    v64 = v.astype(np.float64)
    k = rng.integers(0, len(f), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n) * (1 - 3 * bary_min) + bary_min
    p = np.einsum("ij,ijk->ik", w, v64[f[k]])
    off = off if np.ndim(off) else rng.choice([-off, off], n)
    return p + np.asarray(off)[:, None] * R.face_normals(v, f)[k], k


def _points(v, f, n, seed=0):
    """Surface samples +-0.02 along the normal, uniform in the (enlarged) box, far away, exactly on vertices and edges."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    c, ext = (lo + hi) / 2, (hi - lo).max()
    parts = [_surface(v, f, n // 2, rng, 0.02)[0],
             c + (rng.uniform(-0.7, 0.7, (n // 4, 3)) * ext),
             c + rng.normal(size=(n // 16, 3)) * 20 * ext,
             v[rng.integers(0, len(v), n // 16)].astype(np.float64)]
    e = f[rng.integers(0, len(f), n // 8)]
    t = rng.uniform(0, 1, (len(e), 1)).astype(np.float32)
    parts.append((v[e[:, 0]] * (1 - t) + v[e[:, 1]] * t).astype(np.float64))     # on edges (to fp32 rounding)
    return np.concatenate(parts).astype(np.float32)


def _query(idx, pts, mode, brute):
    p = torch.as_tensor(pts, device=DEV)
    if mode == "unsigned":
        return idx.unsigned_distance(p, return_uvw=True, brute_force=brute)
    return idx.signed_distance(p, return_uvw=True, mode=mode, brute_force=brute)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_grid_equals_brute_force_bit_for_bit(mesh):
    from humangaussian_amd.mesh import MeshIndex
    v, f = MESHES[mesh]()
    idx = MeshIndex(v, f)
    pts = _points(v, f, 6000 if mesh == "icosphere5" else 16000, seed=1)
    for mode in ("raystab", "unsigned"):
        dg, fg, ug = _query(idx, pts, mode, False)
        db, fb, ub = _query(idx, pts, mode, True)
        assert torch.equal(fg, fb), (mode, (fg != fb).sum().item())
        assert _same_bits(dg, db), (mode, (dg != db).sum().item())
        assert _same_bits(ug, ub), mode
        assert fg.dtype == torch.int64 and dg.dtype == ug.dtype == torch.float32 and ug.shape == (len(pts), 3)
        assert (fg >= 0).all() and (ug >= 0).all()
        if mode == "raystab" and mesh in CLOSED:
            assert (dg < 0).any() and (dg > 0).any()


def test_degenerate_face_empty_query_one_face_and_non_finite_points():
    from humangaussian_amd.mesh import MeshIndex
    v, f = R.cube()
    v = np.concatenate([v, np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)])
    f = np.concatenate([np.array([[8, 9, 10]], np.int32), f])      # face 0: collinear, skipped
    idx = MeshIndex(v, f)
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-1, 1, (3000, 3)), [[1.0, 1.0, 1.0], [0.2, 0.2, 0.2]]]).astype(np.float32)
    for brute in (False, True):
        d, fc, uvw = idx.signed_distance(torch.as_tensor(pts, device=DEV), return_uvw=True, mode="raystab", brute_force=brute)
        assert (fc != 0).all() and (fc >= 1).all()
    dg, fg, ug = idx.signed_distance(torch.as_tensor(pts, device=DEV), return_uvw=True, mode="raystab")
    assert torch.equal(fg, fc) and _same_bits(dg, d) and _same_bits(ug, uvw)
    # P = 0, with the points' leading shape
    d0, f0, u0 = idx.signed_distance(torch.zeros(0, 3, device=DEV), return_uvw=True, mode="raystab")
    assert d0.shape == (0,) and f0.shape == (0,) and u0.shape == (0, 3)
    d2, f2, u2 = idx.unsigned_distance(torch.zeros(2, 5, 3, device=DEV), return_uvw=False)
    assert d2.shape == (2, 5) and f2.shape == (2, 5) and u2 is None
    # F = 1: a single triangle, closed form
    one = MeshIndex(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    q = torch.tensor([[0.2, 0.3, 0.5], [-1.0, -2.0, 0.0], [1.0, 1.0, -1.0]], device=DEV)
    for brute in (False, True):
        d, fc, uvw = one.signed_distance(q, return_uvw=True, mode="raystab", brute_force=brute)
        assert fc.tolist() == [0, 0, 0]
        np.testing.assert_allclose(d.cpu().numpy(), [0.5, math.sqrt(5.0), math.sqrt(1.5)], rtol=1e-6)   # open: outside
        np.testing.assert_allclose(uvw.cpu().numpy(), [[0.5, 0.2, 0.3], [1, 0, 0], [0, 0.5, 0.5]], atol=1e-6)
    # non-finite points: face -1, dist NaN, uvw 0, on both paths
    bad = torch.tensor([[float("nan"), 0, 0], [0, float("inf"), 0], [0.1, 0.1, 0.1]], device=DEV)
    for brute in (False, True):
        d, fc, uvw = idx.signed_distance(bad, return_uvw=True, mode="raystab", brute_force=brute)
        assert fc[:2].tolist() == [-1, -1] and torch.isnan(d[:2]).all() and (uvw[:2] == 0).all() and fc[2] >= 1
    # F = 0 with P > 0 is an argument error; indices outside [0, V) are refused at build time
    empty = MeshIndex(v, np.zeros((0, 3), np.int32))
    assert empty.signed_distance(torch.zeros(0, 3, device=DEV))[0].shape == (0,)
    with pytest.raises(RuntimeError, match="no faces"):
        empty.signed_distance(torch.zeros(4, 3, device=DEV))
    with pytest.raises(RuntimeError, match="outside"):
        MeshIndex(v, np.array([[0, 1, len(v)]], np.int32))


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_against_the_fp64_reference(mesh):
    from humangaussian_amd.mesh import MeshIndex
    v, f = MESHES[mesh]()
    idx = MeshIndex(v, f)
    pts = _points(v, f, 1000 if mesh == "icosphere5" else 2000, seed=2)
    d, fc, uvw = (t.cpu().numpy() for t in _query(idx, pts, "raystab", False))
    d2r, fr, uvwr, d2b = R.closest_point(pts, v, f)
    ext = float((v.max(0) - v.min(0)).max())
    tol = 1e-5 * ext
    dr = np.sqrt(d2r)
    assert np.abs(np.abs(d) - dr).max() <= tol, np.abs(np.abs(d) - dr).max()
    clear = np.sqrt(d2b) - dr > tol
    assert clear.mean() > 0.25                           # (points on vertices and far away tie between faces)
    assert (fc[clear] == fr[clear]).all(), (fc[clear] != fr[clear]).sum()
    assert np.abs(uvw[clear] - uvwr[clear]).max() <= 1e-4
    np.testing.assert_allclose(uvw.sum(1), 1.0, atol=1e-5)
    # the sign: fp64 ray stab (the winding number, equal to it on a closed mesh - test_mesh_query_cpu.py - and cheaper)
    inside = (R.winding_number(pts, v, f) > 0.5) if mesh in CLOSED else R.raystab_inside(pts, v, f)
    far = np.abs(d) > 1e-5
    assert ((d < 0) == inside)[far].all(), ((d < 0) != inside)[far].sum()


def _closed_samples(mesh, n, rng):
    v, f = MESHES[mesh]()
    if mesh == "icosphere5":
        p = rng.normal(size=(n, 3))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        rin, rout = np.cbrt(rng.uniform(0, 1, n)) * 0.998, 1.001 + rng.exponential(0.3, n)
        return v, f, p * rin[:, None], p * rout[:, None]
    if mesh == "cube":
        pin = rng.uniform(-0.4999, 0.4999, (n, 3))
        pout = rng.uniform(-1.5, 1.5, (4 * n, 3))
        return v, f, pin, pout[np.abs(pout).max(1) > 0.5001][:n]
    R_, r_ = 0.6, 0.25                                   # the polygonal torus lies within (r - 0.0045, r + 0.001) of the tube axis
    pts = rng.uniform([-0.9, -0.9, -0.3], [0.9, 0.9, 0.3], (8 * n, 3))
    tube = np.hypot(np.hypot(pts[:, 0], pts[:, 1]) - R_, pts[:, 2])
    return v, f, pts[tube < r_ - 0.006][:n], pts[tube > r_ + 0.002][:n]


@pytest.mark.parametrize("mesh", CLOSED)
def test_closed_meshes_no_ray_slips_through(mesh):
    from humangaussian_amd.mesh import MeshIndex
    rng = np.random.default_rng(4)
    v, f, pin, pout = _closed_samples(mesh, 100_000, rng)
    assert len(pin) == len(pout) == 100_000
    idx = MeshIndex(v, f)
    din = idx.signed_distance(torch.as_tensor(pin, dtype=torch.float32, device=DEV), mode="raystab")[0]
    dout = idx.signed_distance(torch.as_tensor(pout, dtype=torch.float32, device=DEV), mode="raystab")[0]
    assert (din < 0).all(), (din >= 0).sum().item()
    assert (dout > 0).all(), (dout <= 0).sum().item()


def _reference_rebuild(vertices, faces, mapping_dist, mapping_face, mapping_uvw, points):
    """/root/reference/animation.py:345-368 in numpy, as written there."""
    fc = faces[mapping_face]
    v0, v1, v2 = vertices[fc[:, 0]], vertices[fc[:, 1]], vertices[fc[:, 2]]
    fnormals = np.cross(v1 - v0, v2 - v0)
    fnormals = fnormals / (np.linalg.norm(fnormals, axis=1, keepdims=True) + 1e-20)
    cpoints = v0 * mapping_uvw[:, [0]] + v1 * mapping_uvw[:, [1]] + v2 * mapping_uvw[:, [2]]
    rebuilt = cpoints + mapping_dist[:, None] * fnormals
    return np.sqrt(np.sum((rebuilt - points) ** 2, axis=-1))


def test_anchor_round_trip_on_the_icosphere():
    from humangaussian_amd.animation import anchor_to_mesh
    v, f = R.icosphere(5)
    rng = np.random.default_rng(5)
    pts, k = _surface(v, f, 20000, rng, rng.uniform(-0.004, 0.004, 20000), bary_min=0.1)
    pts = pts.astype(np.float32)
    tp = torch.as_tensor(pts, device=DEV)
    anchors, keep, err = anchor_to_mesh(tp, v, f, max_error=0.01)
    assert keep.all() and err.max().item() <= 1e-5, err.max().item()
    assert torch.equal(anchors.mapping_face.long().cpu(), torch.as_tensor(k))
    rebuilt = anchors.positions(torch.as_tensor(v, device=DEV))
    assert (rebuilt - tp).norm(dim=1).max().item() <= 1e-5
    # keep = ~(err > max_error), recomputed in numpy from the returned mapping (with the median error as the bound: about
    # half of the rows culled)
    thr = float(err.median())
    anchors, keep, err = anchor_to_mesh(tp, v, f, max_error=thr)
    assert torch.equal(keep, ~(err > thr)) and 0 < keep.sum().item() < len(pts)
    mf, mu, md = (t.cpu().numpy() for t in (anchors.mapping_face, anchors.mapping_uvw, anchors.mapping_dist))
    e_np = _reference_rebuild(v, f, md, mf, mu, pts[keep.cpu().numpy()])
    assert len(e_np) == keep.sum().item() and (e_np <= thr + 1e-6).all()


def test_reference_call_and_rebuild_give_the_anchor_keep_set():
    import cubvh
    from humangaussian_amd.animation import anchor_to_mesh
    v, f = _humanoid()
    rng = np.random.default_rng(6)
    pts = np.concatenate([_surface(v, f, 15000, rng, rng.uniform(-0.03, 0.03, 15000))[0],
                          rng.uniform(v.min(0) - 0.05, v.max(0) + 0.05, (5000, 3))]).astype(np.float32)
    points = torch.as_tensor(pts, device=DEV)
    BVH = cubvh.cuBVH(v, f)                                               # animation.py:337-341, numpy mesh
    mapping_dist, mapping_face, mapping_uvw = BVH.signed_distance(points, return_uvw=True, mode="raystab")
    mapping_dist = mapping_dist.detach().cpu().numpy()
    mapping_face = mapping_face.detach().cpu().numpy().astype(np.int32)
    mapping_uvw = mapping_uvw.detach().cpu().numpy().astype(np.float32)
    err_ref = _reference_rebuild(v, f, mapping_dist, mapping_face, mapping_uvw, points.cpu().numpy())
    mask = ~(err_ref > 0.01)
    _, keep, err = anchor_to_mesh(points, v, f, max_error=0.01)
    keep = keep.cpu().numpy()
    borderline = np.abs(err_ref - 0.01) < 2e-6                  # (fp32 rounding of two rebuild formulas)
    assert (keep == mask)[~borderline].all(), (keep != mask).sum()
    assert borderline.sum() <= 20 and 0 < (~mask).sum() < len(pts)
    np.testing.assert_allclose(err.cpu().numpy(), err_ref, atol=1e-5)


class _Model:
    """The reference GaussianModel's six tensors and getters (gaussian_model.py:95-115)."""
    active_sh_degree = max_sh_degree = 0

    def __init__(self, xyz, rng):
        P = len(xyz)
        g = lambda *s: torch.as_tensor(rng.normal(size=s).astype(np.float32), device=DEV)  # noqa: E731
        self._xyz = torch.as_tensor(xyz, device=DEV)
        self._features_dc, self._features_rest = g(P, 1, 3) * 0.5, torch.zeros(P, 0, 3, device=DEV)
        self._opacity, self._scaling, self._rotation = g(P, 1), g(P, 3) * 0.2 - 5.0, g(P, 4)

    get_xyz = property(lambda m: m._xyz)
    get_features = property(lambda m: torch.cat((m._features_dc, m._features_rest), dim=1))
    get_opacity = property(lambda m: torch.sigmoid(m._opacity))
    get_scaling = property(lambda m: torch.exp(m._scaling))
    get_rotation = property(lambda m: torch.nn.functional.normalize(m._rotation))


def test_animator_from_rest_pose_prunes_and_renders_like_a_hand_built_one():
    from humangaussian_amd.animation import AvatarAnimator, MeshAnchoredGaussians, anchor_to_mesh, orbit_frame_camera
    v, f = _humanoid()
    rng = np.random.default_rng(8)
    pts = np.concatenate([_surface(v, f, 6000, rng, rng.uniform(-0.01, 0.01, 6000))[0],
                          rng.uniform(v.min(0), v.max(0), (1000, 3))]).astype(np.float32)
    model = _Model(pts, np.random.default_rng(9))
    before = {k: getattr(model, k).clone() for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling",
                                                     "_rotation")}
    anchors, keep, _ = anchor_to_mesh(before["_xyz"], v, f, max_error=0.01)
    anim = AvatarAnimator.from_rest_pose(model, v, f, max_error=0.01, white_background=True, device=DEV)
    assert torch.equal(anim.keep, keep) and 0 < keep.sum().item() < len(pts)
    for k, t in before.items():
        assert torch.equal(getattr(model, k), t[keep]), k
    hand = _Model(pts, np.random.default_rng(9))
    for k, t in before.items():
        setattr(hand, k, t[keep])
    hand_anim = AvatarAnimator(hand, MeshAnchoredGaussians(f, anchors.mapping_face, anchors.mapping_uvw,
                                                           anchors.mapping_dist, device=DEV), white_background=True, device=DEV)
    posed = torch.as_tensor(v, device=DEV) + torch.tensor([0.01, -0.02, 0.03], device=DEV)
    cam = orbit_frame_camera(0, 128, 128, device=DEV)
    a, b = anim.render_frame(posed, cam), hand_anim.render_frame(posed, cam)
    assert torch.equal(a, b) and a.abs().sum().item() > 0


def test_scale_500k_points_on_the_icosphere():
    from humangaussian_amd.mesh import MeshIndex
    v, f = R.icosphere(5)
    rng = np.random.default_rng(10)
    pts = np.concatenate([_surface(v, f, 400_000, rng, rng.uniform(-0.02, 0.02, 400_000))[0],
                          rng.uniform(-1.3, 1.3, (100_000, 3))]).astype(np.float32)
    p = torch.as_tensor(pts, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx = MeshIndex(v, f)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    d, fc, uvw = idx.signed_distance(p, return_uvw=True, mode="raystab")
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert d.shape == (500_000,) and (fc >= 0).all() and torch.isfinite(d).all()
    sub = torch.as_tensor(rng.choice(len(pts), 20_000, replace=False), device=DEV)
    db, fb, ub = idx.signed_distance(p[sub], return_uvw=True, mode="raystab", brute_force=True)
    assert torch.equal(fb, fc[sub]) and _same_bits(db, d[sub]) and _same_bits(ub, uvw[sub])
    print(f"icosphere5 (20480 faces, grid {idx.grid_dims}, {idx.num_refs} refs): build {1e3 * (t1 - t0):.1f} ms "
          f"(incl. upload), raystab 500k points {1e3 * (t2 - t1):.1f} ms (first call)")
