"""GPU tests of the rotation-carrying re-anchoring pass (csrc/bookkeeping.hip: hgs_k_reanchor_rot_bind / _pose, through the
torch binding's `reanchor_rot`, `MeshAnchoredGaussians.bind_rotations` / `positions_and_rotations` and
`AvatarAnimator(repose_rotations=True)`).

Rotations are compared as matrices R(q), so a quaternion's sign never matters.  The yardstick is the fp64 restatement
(tests/reanchor_rot_reference.py); the kernel's largest element error may be at most twice that of the fp32 restatement on
the same inputs, plus 2^-22 (the two differ only in the last places of square roots and divisions) - the shape of
tests/test_gpu_optim.py's criterion.  HGS_WRITE_PROFILES=1 records the measured pairs in profiles/reanchor_rot_parity.json.
Shapes: 40-face triangle soups, P = 1, 255, 256, 257, 1025 Gaussians (either side of one and of four 256-thread
workgroups)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import reanchor_rot_reference as rr
from humangaussian_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SLACK = 2.0 ** -22


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _run(c, vertices, rot_in, bind):
    """-> (xyz, rot) numpy, one launch"""
    xyz, rot = _lib.load_binding().reanchor_rot(_t(vertices), _t(c["faces"]), _t(c["face"]), _t(c["uvw"]), _t(c["dist"]),
                                                _t(rot_in), bind)
    return xyz.cpu().numpy(), rot.cpu().numpy()


def _repose(c, rest, posed):
    base = _run(c, rest, c["rot_raw"], True)[1]
    return base, _run(c, posed, base, False)


@functools.lru_cache(maxsize=None)
def _case(P):
    """the inputs of size P and both restatements of its three poses (computed once, never written to)"""
    c = rr.case(P)
    for name, posed in (("rest", c["vertices"]), ("posed", c["posed"]), ("moved", c["moved"])):
        c["q64_" + name] = rr.repose_fp64(c["vertices"], posed, c["faces"], c["face"], c["rot_raw"])
        c["q32_" + name] = rr.repose_fp32(c["vertices"], posed, c["faces"], c["face"], c["rot_raw"])
    return c


_PAIRS = {}


def _gate(case_id, got, ref32, R64):
    e_hip, e_ref = rr.matrix_error(got, R64), rr.matrix_error(ref32, R64)
    entry = {"hip_max_abs_err": e_hip, "fp32_restatement_max_abs_err": e_ref, "gate": 2 * e_ref + SLACK}
    print(case_id, entry)
    _PAIRS[case_id] = entry
    if os.environ.get("HGS_WRITE_PROFILES"):
        doc = {"what": "per case of tests/test_gpu_reanchor_rot.py: largest element of |R(rot) - R(fp64 restatement)| for "
                       "hgs_reanchor_rot (bind, then pose) and for the fp32 restatement on the same inputs, and the gate "
                       "2 x the second + 2^-22 the first is held to",
               "device": torch.cuda.get_device_name(0), "cases": dict(sorted(_PAIRS.items()))}
        with open(os.path.join(ROOT, "profiles", "reanchor_rot_parity.json"), "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    assert np.isfinite(got).all()
    assert e_hip <= 2 * e_ref + SLACK, (case_id, entry)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------------ 1. positions

@pytest.mark.parametrize("P", rr.SIZES)
def test_positions_have_the_bits_of_reanchor(P):
    c = _case(P)
    for vertices in (c["vertices"], c["posed"], c["moved"]):
        want = _lib.load_binding().reanchor(_t(vertices), _t(c["faces"]), _t(c["face"]), _t(c["uvw"]), _t(c["dist"])).cpu().numpy()
        for bind in (False, True):
            xyz, rot = _run(c, vertices, c["rot_raw"], bind)
            assert xyz.shape == (P, 3) and rot.shape == (P, 4) and xyz.dtype == rot.dtype == np.float32
            assert np.array_equal(_bits(xyz), _bits(want)), bind
    assert np.abs(want.astype(np.float64) - rr.positions_fp64(c["moved"], c["faces"], c["face"], c["uvw"], c["dist"])).max() < 1e-6


def test_no_gaussians_give_empty_tensors():
    c = _case(1)
    b = _lib.load_binding()
    for bind in (False, True):
        xyz, rot = b.reanchor_rot(_t(c["vertices"]), _t(c["faces"]), torch.zeros(0, dtype=torch.int32, device=DEV),
                                  torch.zeros(0, 3, device=DEV), torch.zeros(0, device=DEV), torch.zeros(0, 4, device=DEV), bind)
        assert xyz.shape == (0, 3) and rot.shape == (0, 4) and xyz.device.type == "cuda"


def test_wrong_shapes_and_cpu_tensors_raise():
    c = _case(255)
    b = _lib.load_binding()
    args = [_t(c["vertices"]), _t(c["faces"]), _t(c["face"]), _t(c["uvw"]), _t(c["dist"])]
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        b.reanchor_rot(*args, _t(c["rot_raw"][:-1]), False)
    with pytest.raises(RuntimeError, match="HIP device"):
        b.reanchor_rot(*(a.cpu() for a in args), torch.as_tensor(c["rot_raw"]), False)
    with pytest.raises(RuntimeError):
        b.reanchor_rot(*args, torch.as_tensor(c["rot_raw"]), False)


# ------------------------------------------------------------------------------------------------------ 2 - 4. poses

@pytest.mark.parametrize("P", rr.SIZES)
def test_non_rigid_pose_against_fp64(P):
    c = _case(P)
    base, (_, rot) = _repose(c, c["vertices"], c["posed"])
    _gate(f"nonrigid_P{P}", rot, c["q32_posed"], rr.rotmat(c["q64_posed"]))
    _gate(f"bind_P{P}", base, rr.bind_fp32(c["vertices"], c["faces"], c["face"], c["rot_raw"]),
          rr.rotmat(rr.bind_fp64(c["vertices"], c["faces"], c["face"], c["rot_raw"])))


@pytest.mark.parametrize("P", rr.SIZES)
def test_rigid_pose_carries_the_rotation(P):
    c = _case(P)
    _, (_, rot) = _repose(c, c["vertices"], c["moved"])
    _gate(f"rigid_P{P}", rot, c["q32_moved"], c["Rg"][None] @ rr.rotmat(c["rot_raw"]))
    _gate(f"rigid_vs_restatement_P{P}", rot, c["q32_moved"], rr.rotmat(c["q64_moved"]))


@pytest.mark.parametrize("P", rr.SIZES)
def test_rest_pose_returns_the_rotation_and_keeps_its_length(P):
    c = _case(P)
    _, (_, rot) = _repose(c, c["vertices"], c["vertices"])
    _gate(f"rest_P{P}", rot, c["q32_rest"], rr.rotmat(c["rot_raw"]))
    raw_len = np.linalg.norm(c["rot_raw"].astype(np.float64), axis=1)
    ulp = np.spacing(raw_len.astype(np.float32)).astype(np.float64)
    off = np.abs(np.linalg.norm(rot.astype(np.float64), axis=1) - raw_len) / ulp
    print(f"rest_P{P}: |rot| - |rot_raw| at most {off.max():.2f} ulp")
    assert off.max() <= 8.0


# ------------------------------------------------------------------------------------------------------ 5. degenerate faces

@pytest.mark.parametrize("where", ["rest", "posed", "both"])
def test_degenerate_faces_fall_back_to_the_identity(where):
    d = rr.degenerate_case(where)
    bad = d["bad"]
    assert bad.sum() == 12 and set(d["face"][bad].tolist()) == {40, 41, 42, 43}          # one face of each kind
    base, (xyz, rot) = _repose(d, d["rest"], d["posed"])
    assert np.isfinite(base).all() and np.isfinite(rot).all()
    if where in ("rest", "both"):
        assert np.array_equal(_bits(base[bad]), _bits(d["rot_raw"][bad]))               # r = identity: the product is exact
    if where in ("posed", "both"):
        assert np.array_equal(_bits(rot[bad]), _bits(base[bad]))
    q64 = rr.repose_fp64(d["rest"], d["posed"], d["faces"], d["face"], d["rot_raw"])
    q32 = rr.repose_fp32(d["rest"], d["posed"], d["faces"], d["face"], d["rot_raw"])
    _gate(f"degenerate_{where}", rot, q32, rr.rotmat(q64))
    _gate(f"degenerate_{where}_bad_rows", rot[bad], q32[bad], rr.rotmat(q64[bad]))
    # Gaussians on sound faces do not notice their neighbours
    _, (xyz_s, rot_s) = _repose(d, d["rest_sound"], d["posed_sound"])
    assert np.array_equal(_bits(rot[~bad]), _bits(rot_s[~bad])) and np.array_equal(_bits(xyz[~bad]), _bits(xyz_s[~bad]))
    # positions keep today's behaviour, NaN where today's are NaN
    want = _lib.load_binding().reanchor(_t(d["posed"]), _t(d["faces"]), _t(d["face"]), _t(d["uvw"]), _t(d["dist"])).cpu().numpy()
    assert np.array_equal(xyz, want, equal_nan=True) and np.isfinite(xyz[~bad]).all()


# ------------------------------------------------------------------------------------------------------ 6. determinism

def test_two_runs_are_bit_equal():
    c = _case(1025)
    (b1, (x1, r1)), (b2, (x2, r2)) = _repose(c, c["vertices"], c["posed"]), _repose(c, c["vertices"], c["posed"])
    assert np.array_equal(_bits(b1), _bits(b2)) and np.array_equal(_bits(x1), _bits(x2)) and np.array_equal(_bits(r1), _bits(r2))


# ------------------------------------------------------------------------------------------------------ 7 - 9. the animator

class _Model:
    """The reference GaussianModel's six tensors and getters (gaussian_model.py:95-115), SH degree 0"""
    active_sh_degree = max_sh_degree = 0

    def __init__(self, xyz, features_dc, opacity, scaling, rotation):
        self._xyz, self._features_dc = _t(np.asarray(xyz, np.float32)), _t(features_dc)
        self._features_rest = torch.zeros(len(xyz), 0, 3, device=DEV)
        self._opacity, self._scaling, self._rotation = _t(opacity), _t(scaling), _t(rotation)

    get_xyz = property(lambda m: m._xyz)
    get_features = property(lambda m: torch.cat((m._features_dc, m._features_rest), dim=1))
    get_opacity = property(lambda m: torch.sigmoid(m._opacity))
    get_scaling = property(lambda m: torch.exp(m._scaling))
    get_rotation = property(lambda m: torch.nn.functional.normalize(m._rotation))


def _sheet_model(s):
    xyz = rr.positions_fp64(s["vertices"], s["faces"], s["face"], s["uvw"], s["dist"])
    return _Model(xyz, s["features_dc"], s["opacity"], s["scaling"], s["rot_raw"])


def _sheet_animator(s, **kw):
    from humangaussian_amd.animation import AvatarAnimator, MeshAnchoredGaussians
    anchors = MeshAnchoredGaussians(s["faces"], s["face"], s["uvw"], s["dist"], device=DEV)
    return AvatarAnimator(_sheet_model(s), anchors, white_background=True, device=DEV, **kw)


def _camera(s, c2w):
    from humangaussian_amd.renderer import cameras_from_c2w
    return cameras_from_c2w(c2w[None], s["fovy"], s["H"], s["W"], device=DEV)[0]


@functools.lru_cache(maxsize=None)
def _sheet_distances():
    """-> (D_on, D_off, rest image): the sheet and the camera turned together by 90 degrees, against the rest image"""
    s = rr.sheet_scene()
    rest = _sheet_animator(s).render_frame(_t(s["vertices"]), _camera(s, s["c2w"]))
    on = _sheet_animator(s, repose_rotations=True, rest_vertices=_t(s["vertices"]))
    off = _sheet_animator(s)
    cam = _camera(s, s["c2w_moved"])
    img_on, img_off = on.render_frame(_t(s["moved"]), cam), off.render_frame(_t(s["moved"]), cam)
    assert rest.shape == (3, rr.SHEET_HW, rr.SHEET_HW) and bool(torch.isfinite(img_on).all())
    assert float((1.0 - rest).abs().mean()) > 0.01                                      # the needles are drawn
    assert off.gaussians._rotation.data_ptr() != on.gaussians._rotation.data_ptr()
    return float((img_on - rest).abs().mean()), float((img_off - rest).abs().mean()), rest


def test_a_rigidly_moved_scene_renders_the_rest_image_only_with_the_switch_on():
    """What the feature is for.  200 needles (scales 10 : 1 : 1, SH degree 0, opacity 0.8) on both sides of a small sheet, at
    128 x 128; the mesh turns by 90 degrees about (1, 2, 3) / sqrt(14) and the camera with it, so the scene has moved rigidly
    and the image must be the rest image.  D = mean |image - rest image|.
    oracle/gs_oracle.py on the CPU, rotations and positions from the restatement of the same format:
        fp64:  D_off = 2.033e-02,  D_on = 1.182e-08        fp32:  D_off = 2.033e-02,  D_on = 3.587e-08
    (the fp64 D_on is what the fp32 rounding of the moved vertices and of the moved camera leaves): the oracle clears
    D_on <= D_off / 50 by a further factor of 1e4 in either format, and D_off >= 1e-3 by a factor of 20.
    Measured on an MI355X through the animator:  D_off = 2.033e-02,  D_on = 5.632e-08."""
    d_on, d_off, _ = _sheet_distances()
    print(f"sheet: D_on = {d_on:.3e}, D_off = {d_off:.3e}, D_off / D_on = {d_off / max(d_on, 1e-300):.1f}")
    assert d_off >= 1e-3
    assert d_on <= d_off / 50


def test_the_default_path_is_untouched():
    from humangaussian_amd.animation import AvatarAnimator
    from humangaussian_amd.renderer import Renderer
    s = rr.sheet_scene()
    anim = _sheet_animator(s)
    assert anim.repose_rotations is False and anim.anchors.rot_base is None
    rotation = anim.gaussians._rotation
    kept = rotation.clone()
    cam = _camera(s, s["c2w_moved"])
    frame = anim.render_frame(_t(s["moved"]), cam)
    assert anim.gaussians._rotation is rotation and torch.equal(rotation, kept) and anim.anchors.rot_base is None
    hand = _sheet_model(s)
    with torch.no_grad():
        hand._xyz = anim.anchors.positions(_t(s["moved"]))
        want = Renderer(hand, white_background=True, device=DEV).render(cam)["image"]
    assert torch.equal(frame, want) and torch.equal(anim.gaussians._xyz, hand._xyz)
    with pytest.raises(ValueError, match="rest_vertices"):
        AvatarAnimator(_sheet_model(s), anim.anchors, device=DEV, repose_rotations=True)
    # with the switch on, both tensors are assigned, from one pass
    on = _sheet_animator(s, repose_rotations=True, rest_vertices=s["vertices"])
    on.render_frame(_t(s["moved"]), cam)
    xyz, rot = on.anchors.positions_and_rotations(_t(s["moved"]))
    assert torch.equal(on.gaussians._xyz, xyz) and torch.equal(on.gaussians._rotation, rot)
    assert torch.equal(xyz.view(torch.int32), hand._xyz.view(torch.int32))


def test_from_rest_pose_binds_the_culled_rows_on_the_body_mesh():
    from humangaussian_amd import synth
    from humangaussian_amd.animation import AvatarAnimator, MotionDriver, orbit_frame_camera
    v, f, _ = synth.human_mesh()
    rng = np.random.default_rng(7900)
    n_on, n_off = 3000, 400
    face = rng.integers(0, len(f), n_on)
    on_surface = rr.positions_fp64(v, f, face, rng.dirichlet((1.0, 1.0, 1.0), n_on), rng.uniform(-0.004, 0.004, n_on))
    pts = np.concatenate([on_surface, rng.uniform(v.min(0), v.max(0), (n_off, 3))]).astype(np.float32)
    P = len(pts)
    tensors = dict(features_dc=rng.uniform(-1.5, 1.5, (P, 1, 3)).astype(np.float32),
                   opacity=np.full((P, 1), np.log(0.8 / 0.2), np.float32),
                   scaling=np.log(np.tile(np.array([[0.02, 0.002, 0.002]], np.float32), (P, 1))),
                   rotation=rr.raw_quaternions(P, rng))
    m_on, m_off = _Model(pts, **tensors), _Model(pts, **tensors)
    on = AvatarAnimator.from_rest_pose(m_on, v, f, white_background=True, device=DEV, repose_rotations=True)
    off = AvatarAnimator.from_rest_pose(m_off, v, f, white_background=True, device=DEV)
    kept = int(on.keep.sum())
    assert torch.equal(on.keep, off.keep) and 0 < kept < P
    assert on.anchors.rot_base.shape == (kept, 4) and m_on._rotation.shape == (kept, 4) and off.anchors.rot_base is None
    assert torch.equal(m_on._rotation, _t(tensors["rotation"])[on.keep])
    # the bound rows are the culled model's rows, in order
    want = rr.bind_fp64(v, f, on.anchors.mapping_face.cpu().numpy(), m_on._rotation.cpu().numpy())
    assert np.abs(rr.rotmat(on.anchors.rot_base.cpu().numpy()) - rr.rotmat(want)).max() < 1e-4
    # at the rest pose the re-posed frame is the un-reposed one: its distance against the sheet's D_off, by the sheet's ratio
    cam = orbit_frame_camera(0, 128, 128, device=DEV)
    rest_on, rest_off = on.render_frame(_t(v), cam), off.render_frame(_t(v), cam)
    d_rest = float((rest_on - rest_off).abs().mean())
    _, d_off, _ = _sheet_distances()
    print(f"body mesh at rest: D_on = {d_rest:.3e} against the sheet's D_off = {d_off:.3e}")
    assert float((1.0 - rest_off).abs().mean()) > 1e-3 and d_rest <= d_off / 50
    # a posed frame renders finite, and its rotations have moved
    posed = MotionDriver(v, device=DEV).vertices(5)
    img = on.render_frame(posed, cam)
    assert img.shape == (3, 128, 128) and bool(torch.isfinite(img).all()) and bool(torch.isfinite(m_on._rotation).all())
    assert not torch.equal(m_on._rotation, _t(tensors["rotation"])[on.keep]) and float((1.0 - img).abs().mean()) > 1e-3
