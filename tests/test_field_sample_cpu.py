"""CPU tests of the field's point samples (include/hgs_rast.h: hgs_fsample): the numpy restatement
(tests/field_sample_reference.py) against central differences and a one-colour cloud, the C and Python surface without a
GPU, the mesh PLY writer read back, and the conditions the GPU cases (tests/test_gpu_field_sample.py) rest on, checked on
the restatement alone."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_sample_cases as C  # noqa: E402
import field_sample_reference as SR  # noqa: E402
import fields_reference as FR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wide_cloud(n=150, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32), (0.05 + 0.9 * rng.uniform(size=(n, 1))).astype(np.float32),
            (0.08 * np.exp(0.5 * rng.normal(size=(n, 3)))).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the restatement

def test_restated_gradient_against_central_differences():
    """G = sum o e Sigma^-1 d is minus the gradient of the restated density: central differences at points inside one
    block (both neighbours of a point take the same list)."""
    cloud, res, nb = _wide_cloud(), 16, 2
    P = FR.prepare(*cloud, res, nb, 1.5, np.float64)
    rng = np.random.default_rng(5)
    pts = rng.uniform(0.1, 0.8, size=(200, 3)) * rng.choice([-1.0, 1.0], size=(1, 3))     # one octant = one block
    pts = pts.astype(np.float32)
    s = SR.sample(cloud, pts, None, res, nb, normalized=True, prepared=P)
    assert not s.near.any() and len(np.unique(s.block, axis=0)) == 1 and s.density.min() > 0
    h = 2.0 ** -12                                              # exact in fp32 beside coordinates of this size
    grad = np.zeros((len(pts), 3))
    for a in range(3):
        step = np.zeros(3, np.float32)
        step[a] = h
        up = SR.sample(cloud, pts + step, None, res, nb, normalized=True, prepared=P)
        dn = SR.sample(cloud, pts - step, None, res, nb, normalized=True, prepared=P)
        assert np.array_equal(up.block, s.block) and np.array_equal(dn.block, s.block)
        grad[:, a] = (up.density - dn.density) / (((pts + step)[:, a].astype(np.float64)) - (pts - step)[:, a].astype(np.float64))
    scale = np.abs(s.G).max()
    assert np.abs(-grad - s.G).max() <= 1e-4 * scale, (np.abs(-grad - s.G).max(), scale)      # O(h^2) truncation
    # the normal points from high density to low: a short step along it lowers the density
    ok = np.linalg.norm(s.G, axis=1) > 1e-3 * scale
    ahead = SR.sample(cloud, (pts + 4 * h * s.normal).astype(np.float32), None, res, nb, normalized=True, prepared=P)
    assert (ahead.density[ok] < s.density[ok]).all()
    np.testing.assert_allclose(np.linalg.norm(s.normal[ok], axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("dtype, tol", [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_one_colour_cloud_returns_that_colour_wherever_there_is_density(dtype, tol):
    cloud, res, nb = FR.cloud(300, 8), 16, 8                     # a thin ellipsoid: the outer blocks list nothing
    colour = np.array([0.25, 0.5, 0.875], np.float32)
    pts = np.random.default_rng(2).uniform(-1.1, 1.1, size=(1500, 3)).astype(np.float32)
    s = SR.sample(cloud, pts, np.tile(colour, (300, 1)), res, nb, dtype=dtype, normalized=True)
    has = s.density > 0
    assert has.sum() > 100 and (~has).sum() > 100
    assert (s.color[~has] == 0).all() and (s.normal[~has] == 0).all()
    # (a density made of denormal terms cannot carry a colour: o e c rounds to 0 or to o e)
    normal_range = s.density > 1e-30
    assert normal_range.sum() > 100
    assert np.abs(s.color[normal_range] - colour).max() <= tol
    assert (s.color[has] >= 0).all() and (s.color[has] <= 1 + tol).all()


def test_restated_membership_and_zeros():
    """A point on a grid sample belongs to that sample's block, one ulp below to the block before; points outside the grid
    take the edge blocks; points that are not finite give zeros."""
    cloud, res, nb = _wide_cloud(), 16, 4
    ax = FR.axis_samples(res)
    first = ax[8]                                               # first sample of block 2
    pts = np.array([[first, 0, 0], [np.nextafter(first, np.float32(-2)), 0, 0], [-7, 9, 0.3], [np.nan, 0, 0], [0, np.inf, 0]],
                   np.float32)
    s = SR.sample(cloud, pts, np.ones((150, 3), np.float32), res, nb, normalized=True)
    assert s.block[0, 0] == 2 and s.block[1, 0] == 1 and tuple(s.block[2]) == (0, 3, 2)
    assert s.near[0] and s.near[1] and not s.near[2]
    assert not s.finite[3] and not s.finite[4]
    for a in (s.density, s.normal, s.color):
        assert (a[3:] == 0).all()


# ------------------------------------------------------------------------------------------------ the C surface

def test_c_surface_without_a_gpu():
    from humangaussian_amd import _lib
    _lib.build()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 17 and lib.hgs_abi_version() == 17
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(hgs_fsample\w*)\s*\(", hdr, flags=re.M))
    assert declared == {"hgs_fsample_scratch_bytes", "hgs_fsample"} and declared <= set(_lib.EXPORTS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "hgs_fsample") and hasattr(raw, "hgs_fsample_scratch_bytes")
    # the struct of the header, member by member, against the ctypes mirror (LP64: pointers 8 bytes, int32_t 4)
    body = re.search(r"typedef struct hgs_fsample_args \{(.*?)\} hgs_fsample_args;", hdr, flags=re.S).group(1)
    members = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);", body, flags=re.M)
    assert [m[2] for m in members] == [f[0] for f in _lib.HgsFsampleArgs._fields_]
    size = 0
    for ctype, star, name in members:
        width = 8 if star else {"int32_t": 4}[ctype]
        size = -(-size // width) * width
        assert getattr(_lib.HgsFsampleArgs, name).offset == size, name
        size += width
    assert ctypes.sizeof(_lib.HgsFsampleArgs) == -(-size // 8) * 8 == 88
    # sizing is host arithmetic: monotone in M, 0 for what the call refuses
    sizes = [lib.hgs_fsample_scratch_bytes(m, 16) for m in (0, 1, 255, 256, 257, 100000, 1 << 24)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] >= 8 * (1 << 24)
    assert sizes[5] >= 8 * 100000 + 16 ** 3 * 12 and sizes[5] % 256 == 0
    assert lib.hgs_fsample_scratch_bytes(-1, 16) == 0
    assert lib.hgs_fsample_scratch_bytes(10, 0) == 0 and lib.hgs_fsample_scratch_bytes(10, 33) == 0
    assert lib.hgs_fsample_scratch_bytes(10, 1) > 0 and lib.hgs_fsample_scratch_bytes(10, 32) > 0

    class Info(ctypes.Structure):                                            # hgs_field_info
        _fields_ = [("bmin", ctypes.c_uint32 * 3), ("bmax", ctypes.c_uint32 * 3), ("center", ctypes.c_float * 3),
                    ("extent", ctypes.c_float), ("scale", ctypes.c_float), ("num_kept", ctypes.c_uint32),
                    ("num_gaussians", ctypes.c_int32), ("num_blocks", ctypes.c_int32), ("resolution", ctypes.c_int32),
                    ("grow", ctypes.c_float), ("num_refs", ctypes.c_uint64)]
    assert ctypes.sizeof(Info) == 72
    info = Info(num_kept=5, num_gaussians=10, num_blocks=4, resolution=32, num_refs=100)
    buf = (ctypes.c_float * 64)()                                            # stands for any non-NULL pointer: nothing is read
    ptr = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        a = _lib.HgsFsampleArgs(info_host=ctypes.cast(ctypes.pointer(info), ctypes.c_void_p), axis=ptr, plan=ptr, lists=ptr,
                                M=4, normalized=0, points=ptr, colors=ptr, scratch=ptr, density=ptr, normal=ptr, color=ptr)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.hgs_fsample(ctypes.byref(a), None)

    assert lib.hgs_fsample(None, None) == -1                                 # a null block
    assert call(M=-1) == -1
    assert call(colors=None) == -1                                           # color without colors
    assert call(info_host=None) == -1
    info.resolution = 33                                                     # an unusable info (33 % 4 != 0)
    assert call() == -1
    info.resolution = 32
    assert call(points=None) == -1 and call(scratch=None) == -1 and call(lists=None) == -1 and call(axis=None) == -1
    assert call(M=0) == 0                                                    # launches nothing
    assert call(M=0, points=None, scratch=None) == 0
    assert call(density=None, normal=None, color=None) == 0                  # nothing asked for
    b = _lib.load_binding()
    assert callable(b.field_build) and callable(b.field_sample)


# ------------------------------------------------------------------------------------------------ save_mesh_ply

@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_save_mesh_ply_reads_back(tmp_path, with_normals, with_colors):
    from humangaussian_amd.ply_io import save_mesh_ply
    rng = np.random.default_rng(4)
    v = rng.normal(size=(7, 3)).astype(np.float32)
    f = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    n = rng.normal(size=(7, 3)).astype(np.float32)
    c = rng.uniform(0, 1, size=(7, 3)).astype(np.float32)
    c[0] = (-0.5, 1.5, 0.5)                                                  # outside [0, 1]: saturates
    c[1] = (0.0, 1.0, 0.498)                                                 # 0.498 * 255 = 126.99 -> 127
    path = str(tmp_path / "mesh.ply")
    save_mesh_ply(path, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n) if with_normals else None,
                  c if with_colors else None)
    rv, rf, names = C.read_mesh_ply(path)
    assert names == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["red", "green", "blue"] if with_colors else [])
    assert np.array_equal(np.stack([rv["x"], rv["y"], rv["z"]], 1), v) and np.array_equal(rf, f)
    if with_normals:
        assert np.array_equal(np.stack([rv["nx"], rv["ny"], rv["nz"]], 1), n)
    if with_colors:
        got = np.stack([rv["red"], rv["green"], rv["blue"]], 1)
        assert got.dtype == np.uint8
        assert np.array_equal(got, np.rint(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8))
        assert tuple(got[0]) == (0, 255, 128) and tuple(got[1]) == (0, 255, 127)
    with pytest.raises(ValueError):
        save_mesh_ply(path, v, f, normals=n[:3])
    with pytest.raises(ValueError):
        save_mesh_ply(path, v, f, colors=c[:3])
    save_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3)), np.zeros((0, 3)))
    rv, rf, _ = C.read_mesh_ply(path)
    assert len(rv) == 0 and len(rf) == 0


# ------------------------------------------------------------------------------------------------ the Python surface

def test_python_surface_without_a_gpu():
    import inspect
    from humangaussian_amd import fields
    assert [(p.name, p.default) for p in inspect.signature(fields.GaussianField.__init__).parameters.values()][2:] == [
        ("resolution", 128), ("num_blocks", 16), ("relax_ratio", 1.5)]
    assert [(p.name, p.default) for p in inspect.signature(fields.GaussianField.sample).parameters.values()][2:] == [
        ("colors", None), ("normalized", False)]
    assert [(p.name, p.default) for p in inspect.signature(fields.extract_mesh_attributes).parameters.values()][1:] == [
        ("density_thresh", 1), ("resolution", 128), ("colors", None)]
    cpu = (torch.zeros(4, 3), torch.ones(4, 1), torch.ones(4, 3), torch.ones(4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        fields.GaussianField(cpu)
    with pytest.raises(RuntimeError, match="HIP device"):
        fields.extract_mesh_attributes(cpu)
    with pytest.raises(ValueError, match="multiple of num_blocks"):
        fields.GaussianField(cpu, resolution=100, num_blocks=16)
    with pytest.raises(ValueError, match="at least 1"):
        fields.GaussianField(cpu, resolution=32, num_blocks=0)
    with pytest.raises(ValueError):
        fields.GaussianField(cpu[:3])
    # sample checks its arguments before it touches the field (a bare instance): shapes first, then the device
    f = object.__new__(fields.GaussianField)
    f.num_gaussians, f._state = 4, None
    with pytest.raises(RuntimeError, match="HIP device"):
        f.sample(torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        f.sample(torch.zeros(5, 3), colors=torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"points must be \(M, 3\)"):
        f.sample(torch.zeros(5, 2))
    with pytest.raises(ValueError, match=r"points must be \(M, 3\)"):
        f.sample(torch.zeros(5))
    with pytest.raises(ValueError, match="one row per Gaussian"):
        f.sample(torch.zeros(5, 3), colors=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="one row per Gaussian"):
        f.sample(torch.zeros(5, 3), colors=torch.zeros(4, 4))

    class _Model:
        _features_dc = torch.tensor([[[0.0, 1.0, -3.0]], [[2.0, -1.0, 0.5]]])

    col = fields.gaussian_colors(_Model())
    want = np.maximum(0.28209479177387814 * _Model._features_dc[:, 0].numpy().astype(np.float64) + 0.5, 0)
    assert col.shape == (2, 3) and np.abs(col.numpy() - want).max() <= 1e-7 and col[0, 2] == 0
    assert "view" in fields.gaussian_colors.__doc__ and "NOT baked" in fields.gaussian_colors.__doc__


# ------------------------------------------------------------------------------------------------ conditions of the GPU cases

@pytest.mark.parametrize("case", C.CASES)
def test_gpu_case_points_stay_under_the_near_cap(case):
    """World points within 1e-6 of a plane between two blocks are not compared on the GPU, and their share of a case's
    points is capped at 0.1 %.  The uniform points must satisfy that by themselves, in both coordinate forms.  The mesh's
    vertices cannot: a marching-cubes vertex lies on a grid edge, so two of its three coordinates are grid samples, and
    with `split` samples per block about 2 / split of the vertices lie on such a plane by construction (measured: 42 %,
    24 % and 48 % of the three meshes).  They are therefore compared in NORMALISED coordinates - all of them, where
    membership is exact - and in world coordinates only off the planes; this holds the meshes to leaving enough vertices
    off the planes for that."""
    cloud, res, nb = C.cloud_of(case)
    v, f, P = C.restated_mesh(case)
    assert len(v) >= 50 and len(f) >= 100, (len(v), len(f))
    uni = C.uniform_points(case)
    assert C.on_plane(uni, P).mean() <= C.NEAR_CAP
    world = C.to_world(uni, P.center, P.scale)
    back = (world.astype(np.float64) - P.center) * P.scale
    assert C.on_plane(back, P).mean() <= C.NEAR_CAP
    assert np.abs(uni) .max() > 1.0 and (np.abs(uni).max(1) <= 1.0).mean() > 0.5       # outside the grid and inside it
    vn = C.vertices_normalised(v, res)
    on = C.on_plane(vn, P)
    print(f"{case}: {len(v)} vertices, {on.mean():.3f} of them on a plane between two blocks")
    assert (~on).sum() >= 40


def test_restated_vertex_normals_agree_with_the_faces_of_the_ellipsoid():
    """The GPU mesh test asks 99 % of the faces to agree with their vertex normals; the cloud must give that by itself."""
    cloud, res, nb = C.ellipsoid_cloud(), C.ELLIPSOID["resolution"], C.ELLIPSOID["num_blocks"]
    occ, P = FR.field(*cloud, resolution=res, num_blocks=nb, dtype=np.float64)
    v, f = FR.weld(FR.marching_cubes(occ, C.threshold(occ.max())))
    assert len(f) > 500
    s = SR.sample(cloud, C.vertices_normalised(v, res), C.two_colours(cloud), res, nb, normalized=True, prepared=P)
    share = SR.face_agreement(v, f, s.normal)
    print(f"ellipsoid: {len(v)} vertices, {len(f)} faces, {share:.4f} agree with their vertex normals")
    assert share >= 0.99
    # ... and the two-coloured version of it (upper half red, lower half blue) shows its colours away from the seam
    world = C.to_world(C.vertices_normalised(v, res), P.center, P.scale)
    far = C.far_from_seam(world, cloud)
    assert (far != 0).sum() >= 0.3 * len(v) and (far > 0).any() and (far < 0).any()
    err = np.abs(s.color - np.where((far > 0)[:, None], C.RED, C.BLUE))[far != 0].max()
    print(f"two colours: {(far != 0).sum()} of {len(v)} vertices beyond three standard deviations, largest error {err:.2e}")
    assert err <= 0.05
