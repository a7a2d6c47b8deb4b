"""CPU tests of the rotation-carrying re-anchoring pass: the properties of its numpy restatement
(tests/reanchor_rot_reference.py) in fp64, the C entry point's argument checks on the built library (no launch: there is
no GPU here), and the Python layer's error before `bind_rotations`."""
import ctypes

import numpy as np
import pytest

import reanchor_rot_reference as rr
from humangaussian_amd import _lib


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def case():
    return rr.case(257)


def test_rigid_motion_carries_the_rotation_matrix(case):
    c = case
    # (the moved vertices stay fp64 here: `rigid()` would round them to fp32, which is not the restatement's error)
    a, b, cc = (c["vertices"].astype(np.float64)[c["faces"][c["face"]][:, k]] for k in range(3))
    moved = [p @ c["Rg"].T + c["t"] for p in (a, b, cc)]
    base = rr.hamilton(rr.conj(rr.face_quat(a, b, cc)), c["rot_raw"].astype(np.float64))
    rot = rr.hamilton(rr.face_quat(*moved), base)
    want = c["Rg"][None] @ rr.rotmat(c["rot_raw"])
    assert np.abs(rr.rotmat(rot) - want).max() <= 1e-12


def test_rest_pose_returns_the_raw_rotation_and_lengths_are_kept(case):
    c = case
    rot = rr.repose_fp64(c["vertices"], c["vertices"], c["faces"], c["face"], c["rot_raw"])
    assert np.abs(rr.rotmat(rot) - rr.rotmat(c["rot_raw"])).max() <= 1e-12
    posed = rr.repose_fp64(c["vertices"], c["posed"], c["faces"], c["face"], c["rot_raw"])
    raw_len = np.linalg.norm(c["rot_raw"].astype(np.float64), axis=1)
    for q in (rot, posed, rr.bind_fp64(c["vertices"], c["faces"], c["face"], c["rot_raw"])):
        assert np.abs(np.linalg.norm(q, axis=1) / raw_len - 1).max() <= 1e-12
    # the posed frames differ from the rest frames (the case does move), and the face quaternions are unit
    assert np.abs(rr.rotmat(posed) - rr.rotmat(c["rot_raw"])).max() > 1e-2
    a, b, cc = rr._corners(c["posed"], c["faces"], c["face"], np.dtype(np.float64))
    r = rr.face_quat(a, b, cc)
    assert np.abs(np.linalg.norm(r, axis=1) - 1).max() <= 1e-12
    F = rr.rotmat(r)
    e1 = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
    n = np.cross(b - a, cc - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(F[:, :, 0] - e1).max() <= 1e-12 and np.abs(F[:, :, 2] - n).max() <= 1e-12
    assert np.abs(F[:, :, 1] - np.cross(n, e1)).max() <= 1e-12


def test_every_branch_of_the_conversion_is_a_quaternion_of_the_frame():
    """faces whose frames are near each of the four half-turn cases (w, x, y or z largest)"""
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        Rm = rr.random_rotation(rng)
        a = rng.uniform(-0.5, 0.5, 3)
        b, c = a + 0.05 * Rm[:, 0], a + 0.03 * Rm[:, 0] + 0.04 * Rm[:, 1]
        for dt, tol in ((np.float64, 1e-12), (np.float32, 2e-6)):
            q = rr.face_quat(*(p[None].astype(dt) for p in (a, b, c)))
            assert q.dtype == dt and np.abs(rr.rotmat(q)[0] - Rm).max() <= tol
        seen.add(int(np.argmax(np.abs(q[0]))))
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("where", ["rest", "posed", "both"])
def test_degenerate_rules(where):
    d = rr.degenerate_case(where)
    bad = d["bad"]
    for bind, pose, dt in ((rr.bind_fp64, rr.pose_fp64, np.float64), (rr.bind_fp32, rr.pose_fp32, np.float32)):
        base = bind(d["rest"], d["faces"], d["face"], d["rot_raw"])
        rot = pose(d["posed"], d["faces"], d["face"], base)
        assert np.isfinite(base).all() and np.isfinite(rot).all()
        raw = d["rot_raw"].astype(dt)
        if where in ("rest", "both"):
            assert np.array_equal(base[bad], raw[bad])                       # r = identity: the product is exact
        if where in ("posed", "both"):
            assert np.array_equal(rot[bad], base[bad])
        # every kind is caught, in both formats
        a, b, c = rr._corners(d["rest" if where != "posed" else "posed"], d["faces"], d["face"], np.dtype(dt))
        r = rr.face_quat(a, b, c)
        assert np.array_equal(r[bad], np.tile(np.array([1, 0, 0, 0], dt), (int(bad.sum()), 1)))
        assert not np.array_equal(r[~bad], np.tile(np.array([1, 0, 0, 0], dt), (int((~bad).sum()), 1)))
        # Gaussians on sound faces do not notice
        sound = pose(d["posed_sound"], d["faces"], d["face"], bind(d["rest_sound"], d["faces"], d["face"], d["rot_raw"]))
        assert np.array_equal(rot[~bad], sound[~bad])


def test_the_meshes_are_what_the_tests_say():
    v, f = rr.triangle_soup(7257)
    assert f.shape == (rr.NUM_FACES, 3) and v.dtype == np.float32
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    edges = np.stack([np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1)], 1)
    assert edges.min() >= rr.EDGE_MIN and edges.max() <= rr.EDGE_MAX
    assert min(min(rr._angles(a[k], b[k], c[k])) for k in range(len(f))) >= rr.ANGLE_MIN
    cse = rr.case(1025)
    assert set(cse["face"].tolist()) == set(range(rr.NUM_FACES))
    norms = np.linalg.norm(cse["rot_raw"], axis=1)
    assert norms.min() < 0.5 and norms.max() > 3.0                           # deliberately not unit
    moved = np.linalg.norm(cse["posed"].astype(np.float64) - cse["vertices"], axis=1)
    assert 0 < moved.max() <= 0.3 * rr.EDGE_MAX + 1e-6


def test_c_entry_point_checks_its_arguments(lib):
    assert "hgs_reanchor_rot" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "hgs_reanchor_rot")
    fn = lib.hgs_reanchor_rot
    p = ctypes.c_void_p(64)                                    # never dereferenced: every call below returns before a launch
    args = [p] * 6                                             # vertices, faces, mapping_face, mapping_uvw, mapping_dist, rot_in
    assert fn(0, *([None] * 6), 0, None, None, None) == 0      # P == 0: HGS_OK, no launch
    assert fn(0, *([None] * 6), 1, None, None, None) == 0
    assert fn(-1, *args, 0, p, p, None) == -1                  # HGS_EINVAL
    assert fn(-1, *args, 1, p, p, None) == -1
    for k in range(6):
        holed = list(args)
        holed[k] = None
        assert fn(4, *holed, 0, p, p, None) == -1, k
        assert fn(4, *holed, 1, None, p, None) == -1, k
    assert fn(4, *args, 0, p, None, None) == -1                # rot_out
    assert fn(4, *args, 1, None, None, None) == -1
    assert fn(4, *args, 0, None, p, None) == -1                # the pose form writes xyz; the bind form may leave it out


def test_abi_version_stays_17(lib):
    assert lib.hgs_abi_version() == 17 and _lib.ABI_VERSION == 17


def test_rotations_before_bind_raise():
    from humangaussian_amd.animation import MeshAnchoredGaussians
    v, f = rr.triangle_soup(1, num_faces=2)
    anchors = MeshAnchoredGaussians(f, [0, 1], np.full((2, 3), 1 / 3, np.float32), np.zeros(2, np.float32), device="cpu")
    assert anchors.rot_base is None
    with pytest.raises(RuntimeError, match="bind_rotations"):
        anchors.positions_and_rotations(v)
    with pytest.raises(ValueError, match="rotation_raw"):
        anchors.bind_rotations(v, np.zeros((3, 4), np.float32))


def test_the_switch_defaults_to_off():
    import inspect
    from humangaussian_amd.animation import AvatarAnimator
    assert inspect.signature(AvatarAnimator.__init__).parameters["repose_rotations"].default is False
