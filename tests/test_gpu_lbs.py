"""GPU tests of the skinned body (csrc/lbs.hip, humangaussian_amd/body.py, animation.SMPLXDriver).

What the kernels are held to (tests/lbs_reference.py): max |error| over vertices and joints against the float64
restatement <= 4 x the float32 restatement's own max error on the same case, with a floor of 16 eps32 max|v|.  The factor
4 is a margin for the kernel's partition of the two sums (the K rows in 32 slices and a fixed tree; the joints of a vertex
as a packed list), not a measured bound.  Shapes are the smallest that reach every branch of the two kernels; the table
below names the chunk sizes they are built around.  HGS_WRITE_PROFILES=1 records the per-case ratios in
profiles/lbs_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import lbs_reference as lr
import mesh_reference as mr
from humangaussian_amd import _lib, body
from humangaussian_amd.animation import AvatarAnimator, MeshAnchoredGaussians, SMPLXDriver, orbit_frame_camera

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

# ---- the chunk sizes of csrc/lbs.hip -----------------------------------------------------------------------------------
VERTS_PER_THREAD = 4         # a thread of the sweep owns four vertices: three 16-byte loads per row of posedirs
VERTS_PER_WAVE = 64          # 16 lanes x 4 vertices; the four 16-lane groups of a wave are four k-slices of the SAME vertices
VERTS_PER_WORKGROUP = 64     # HGS_LBS_VERTS: the eight waves of a workgroup are 32 k-slices of the same 64 vertices
FRAME_TILE = _lib.LBS_FRAME_TILE   # T: frames that share every load of posedirs (hgs_k_lbs_skin_f8; F = 1: hgs_k_lbs_skin_f1)
K_SLICES = 32                # rows k = slice (mod 32): K = 9 (2 - 1) = 9 leaves 23 slices empty, K = 486 / 567 fill them unevenly
CASES = lr.sweep_cases(VERTS_PER_THREAD, VERTS_PER_WAVE, VERTS_PER_WORKGROUP, FRAME_TILE)
# V: 1 3 4 5 63 64 65 127 128 129 255 256 257 | J: 1 2 55 64, chain / star / SMPL-X | width: 1 4 5 J | K: 0, 9 (J - 1)
# F: 1 2 T T+1 136 | poses: zero, |a| = 1e-6, random up to pi, one joint at exactly pi | with and without transl / centre+scale


def _body_of(case, built):
    b = built["body"]
    return body.SkinnedBody(b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"], shapedirs=b["shapedirs"],
                            posedirs=b["posedirs"], betas=built["betas"], device=DEV)


def _finite(*tensors):
    for t in tensors:
        assert bool(torch.isfinite(t).all()), "NaN or Inf in the output"


_RATIOS = {}


def _record(case_id, entry):
    _RATIOS[case_id] = entry
    if not os.environ.get("HGS_WRITE_PROFILES"):
        return
    doc = {"what": "per case of tests/test_gpu_lbs.py: max |error| of hgs_lbs_pose (vertices and joints) against the float64 "
                   "restatement, the float32 restatement's own error, both in units of eps32 max|v|, and the gate "
                   "max(4 ref, 16) the first is held to",
           "device": torch.cuda.get_device_name(0), "cases": dict(sorted(_RATIOS.items()))}
    with open(os.path.join(ROOT, "profiles", "lbs_parity.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_boundary_sweep_against_fp64(case):
    c = lr.build_case(case)
    sb = _body_of(case, c)
    assert sb.weight_width == case["width"] and sb.num_pose_rows == (9 * (case["J"] - 1) if case["pose_blend"] else 0)
    v, j = sb.pose(c["poses"], transl=c["transl"], centre=c["centre"], scale=c["scale"], return_joints=True)
    assert v.shape == (case["F"], case["V"], 3) and j.shape == (case["F"], case["J"], 3) and v.device.type == "cuda"
    _finite(v, j)
    err = max(float(np.abs(v.cpu().numpy().astype(np.float64) - c["v64"]).max()),
              float(np.abs(j.cpu().numpy().astype(np.float64) - c["j64"]).max()))
    unit = lr.EPS32 * c["vmax"]
    gate = max(4.0 * c["ref_err"], 16.0 * unit)
    entry = {"hip_over_unit": err / unit, "ref_over_unit": c["ref_err"] / unit, "gate_over_unit": gate / unit,
             "hip_over_ref": err / c["ref_err"] if c["ref_err"] > 0 else (0.0 if err == 0 else float("inf"))}
    print(case["id"], entry)
    _record(case["id"], entry)
    assert err <= gate, (case["id"], entry)


def test_zero_pose_is_the_shaped_template():
    """no rotation, no pose blend: v = sum_j w_j (v_shaped - J_j + J_j') - with one-hot weights on the root, v_shaped exactly"""
    b = lr.make_body(130, 55, "smplx", 1, True, seed=70)
    b["weights"][:] = 0.0
    b["weights"][:, 0] = 1.0
    sb = body.SkinnedBody(b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"], posedirs=b["posedirs"],
                          device=DEV)
    v, j = sb.pose(np.zeros((FRAME_TILE + 1, 55, 3), np.float32), return_joints=True)
    assert torch.equal(v, sb.v_shaped[None].expand_as(v))
    assert float((j - sb.J_rest[None]).abs().max()) <= 64 * lr.EPS32 * float(sb.J_rest.abs().max())
    _finite(v, j)


def _case_named(F, V=257):
    return next(c for c in CASES if c["F"] == F and c["V"] == V and c["J"] == 55 and c["pose_blend"] and c["poses"] == "random")


def test_two_calls_with_the_same_inputs_are_bit_equal():
    case = _case_named(FRAME_TILE + 1)
    c = lr.build_case(case)
    sb = _body_of(case, c)
    kw = dict(transl=c["transl"], centre=c["centre"], scale=c["scale"], return_joints=True)
    v1, j1 = sb.pose(c["poses"], **kw)
    v2, j2 = sb.pose(c["poses"], **kw)
    assert torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(j1.view(torch.int32), j2.view(torch.int32))
    _finite(v1, j1)


@pytest.mark.parametrize("F", [FRAME_TILE + 1, 136])
def test_frame_of_a_batch_is_bit_equal_to_its_single_frame_call(F):
    case = _case_named(F)
    c = lr.build_case(case)
    sb = _body_of(case, c)
    poses = torch.from_numpy(c["poses"]).to(DEV)
    transl = torch.from_numpy(c["transl"]).to(DEV)
    vb, jb = sb.pose(poses, transl=transl, centre=c["centre"], scale=c["scale"], return_joints=True)
    _finite(vb, jb)
    frames = range(F) if F <= 16 else (0, 1, 7, 8, 9, 63, 64, 127, 128, 134, 135)
    for f in frames:
        v1, j1 = sb.pose(poses[f], transl=transl[f], centre=c["centre"], scale=c["scale"], return_joints=True)
        assert v1.shape == (1, case["V"], 3)
        assert torch.equal(v1[0].view(torch.int32), vb[f].view(torch.int32)), f
        assert torch.equal(j1[0].view(torch.int32), jb[f].view(torch.int32)), f


# ------------------------------------------------------------------------------------------------------- end to end

class _Model:
    """The reference GaussianModel's six tensors and getters (gaussian_model.py:95-115)."""
    active_sh_degree = max_sh_degree = 0

    def __init__(self, xyz, rng):
        P = len(xyz)
        g = lambda *s: torch.as_tensor(rng.normal(size=s).astype(np.float32), device=DEV)  # noqa: E731
        self._xyz = torch.as_tensor(xyz, device=DEV)
        self._features_dc, self._features_rest = g(P, 1, 3) * 0.5, torch.zeros(P, 0, 3, device=DEV)
        self._opacity, self._scaling, self._rotation = g(P, 1), g(P, 3) * 0.2 - 4.0, g(P, 4)

    get_xyz = property(lambda m: m._xyz)
    get_features = property(lambda m: torch.cat((m._features_dc, m._features_rest), dim=1))
    get_opacity = property(lambda m: torch.sigmoid(m._opacity))
    get_scaling = property(lambda m: torch.exp(m._scaling))
    get_rotation = property(lambda m: torch.nn.functional.normalize(m._rotation))


_E2E = {}


def _end_to_end():
    """a body of 162 vertices (an icosphere stretched to a trunk), 55 joints, a clip of 12 frames - built once"""
    if _E2E:
        return _E2E
    v, f = mr.icosphere(2)
    v = (v * np.array([0.25, 0.8, 0.2])).astype(np.float32)
    b = lr.make_body(len(v), 55, "smplx", 4, True, seed=80, mesh=(v, f))
    rng = np.random.default_rng(81)
    clip = lr.make_poses("random", 12, 55, seed=82) * np.float32(0.3)
    sb = body.SkinnedBody(b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"], posedirs=b["posedirs"],
                          device=DEV)
    n = 3000
    face = rng.integers(0, len(f), n).astype(np.int32)
    uvw = rng.dirichlet([1.0, 1.0, 1.0], n).astype(np.float32)
    dist_ = rng.uniform(-0.004, 0.004, n).astype(np.float32)
    anchors = MeshAnchoredGaussians(f, face, uvw, dist_, device=DEV)
    _E2E.update(b=b, sb=sb, clip=clip, anchors=anchors, n=n)
    return _E2E


def _reference_of_driver(e, body_only, frames):
    """the float64 restatement of what SMPLXDriver computes: the clip's joints 1-21, the zero pose's box as the affine"""
    b, clip = e["b"], e["clip"]
    v_shaped, J_rest = lr.setup(b)
    args = (v_shaped.astype(np.float32), J_rest.astype(np.float32), b["parents"], b["weights"], b["posedirs"])
    rest, _ = lr.pose(*args, np.zeros((1, 55, 3)))
    vmin, vmax = rest[0].min(0), rest[0].max(0)
    centre, scale = (vmax + vmin) / 2, 0.6 / np.max(vmax - vmin) * 1.1 ** 10
    used = np.zeros_like(clip)
    if body_only:
        used[:, 1:22] = clip[:, 1:22]
    else:
        used[:] = clip
    p = used[[i % len(clip) for i in frames]]
    kw = dict(centre=centre.astype(np.float32), scale=float(np.float32(scale)))
    v64, _ = lr.pose(*args, p, dtype=np.float64, **kw)
    v32, _ = lr.pose(*args, p, dtype=np.float32, **kw)
    return centre, scale, used, v64, float(np.abs(v32 - v64).max())


def test_driver_reproduces_the_reference_convention():
    e = _end_to_end()
    drv = SMPLXDriver(e["sb"], e["clip"], body_only=True)
    assert drv.num_poses == 12 and isinstance(drv.source, str)
    centre, scale, used, v64, ref_err = _reference_of_driver(e, True, range(12))
    # centre and scale: the reference's formula (animation.py:321-330) on the zero pose, fixed afterwards
    # (from fp32 vertices that are each within the sweep's floor of the float64 ones)
    slack = 16 * lr.EPS32 * float(np.abs(e["b"]["v_template"]).max() + 1.0)
    assert np.abs(drv.centre - centre).max() <= slack and abs(drv.scale / scale - 1) <= 2 * slack * scale / 1.1 ** 10 / 0.6 + 4 * lr.EPS32
    # body_only: joints 0 and 22+ stay unposed, 1-21 are the clip's
    assert torch.equal(drv.poses.cpu(), torch.from_numpy(used))
    assert float(drv.poses[:, 0].abs().max()) == 0 and float(drv.poses[:, 22:].abs().max()) == 0 and float(drv.poses[:, 1:22].abs().max()) > 0
    every = SMPLXDriver(e["sb"], e["clip"], body_only=False)
    assert torch.equal(every.poses.cpu(), torch.from_numpy(e["clip"])) and every.centre.tolist() == drv.centre.tolist()
    # precompute = the stacked vertices(i), bit for bit; frame i uses pose i mod 12
    frames = [0, 1, 5, 11, 12, 13, 7, 7, 3]
    batch = drv.precompute(frames)
    assert batch.shape == (len(frames), e["sb"].num_vertices, 3)
    _finite(batch)
    for k, i in enumerate(frames):
        assert torch.equal(batch[k].view(torch.int32), drv.vertices(i).view(torch.int32)), (k, i)
    assert torch.equal(drv.vertices(13), drv.vertices(1))
    # the vertices against the float64 restatement of the same convention, within the gate of the sweep
    got = torch.stack([drv.vertices(i) for i in range(12)]).cpu().numpy().astype(np.float64)
    vmax = float(np.abs(v64).max())
    err, gate = float(np.abs(got - v64).max()), max(4 * ref_err, 16 * lr.EPS32 * vmax)
    print("driver: err / unit", err / (lr.EPS32 * vmax), "gate / unit", gate / (lr.EPS32 * vmax))
    assert err <= gate
    # the affine puts the zero pose's box at the origin with its largest side 0.6 * 1.1 ** 10
    rest = e["sb"].pose(np.zeros((55, 3), np.float32), centre=drv.centre, scale=drv.scale)[0]
    assert torch.equal(rest, drv.rest_vertices())
    side = (rest.max(0).values - rest.min(0).values).max().item()
    assert abs(side / (0.6 * 1.1 ** 10) - 1) < 1e-5 and float((rest.max(0).values + rest.min(0).values).abs().max()) < 1e-5


def test_driver_to_animator_renders_and_reanchors_like_the_reference_vertices():
    e = _end_to_end()
    drv = SMPLXDriver(e["sb"], e["clip"], body_only=True)
    anchors = e["anchors"]
    _, _, _, v64, ref_err = _reference_of_driver(e, True, range(12))
    vmax = float(np.abs(v64).max())
    gate = max(4 * ref_err, 16 * lr.EPS32 * vmax)
    for i in (0, 5, 11):
        got = anchors.positions(drv.vertices(i))
        want = anchors.positions(torch.from_numpy(v64[i].astype(np.float32)).to(DEV))
        _finite(got)
        err = float((got.double() - want.double()).abs().max())
        print("frame", i, "re-anchored err / unit", err / (lr.EPS32 * vmax), "gate / unit", gate / (lr.EPS32 * vmax))
        assert err <= gate, (i, err, gate)
    xyz0 = anchors.positions(drv.vertices(0))
    anim = AvatarAnimator(_Model(xyz0.cpu().numpy(), np.random.default_rng(83)), anchors, white_background=True, device=DEV)
    cam = orbit_frame_camera(0, 96, 96, device=DEV)
    a, b = anim.render_frame(drv.vertices(0), cam), anim.render_frame(drv.vertices(5), cam)
    assert a.shape == (3, 96, 96)
    _finite(a, b)
    assert float((1.0 - a).abs().sum()) > 0 and not torch.equal(a, b)         # something is drawn, and the pose moves it
    assert torch.equal(anim.gaussians._xyz, anchors.positions(drv.vertices(5)))


def test_model_file_on_the_device(tmp_path):
    """`from_smplx_npz` ends in the same body as the constructor given the file's arrays"""
    b = lr.make_body(70, 55, "smplx", 4, True, seed=90)
    rng = np.random.default_rng(91)
    shapedirs = (rng.standard_normal((70, 3, 20)) * 0.03).astype(np.float32)
    kintree = np.stack([b["parents"].astype(np.int64) % (1 << 32), np.arange(55)]).astype(np.uint32)
    path = os.path.join(tmp_path, "SMPLX_NEUTRAL.npz")
    np.savez(path, v_template=b["v_template"], f=b["faces"].astype(np.uint32), kintree_table=kintree, J_regressor=b["J_regressor"],
             weights=b["weights"], shapedirs=shapedirs, posedirs=b["posedirs"].T.reshape(70, 3, 486))
    betas, expr = rng.standard_normal(10), rng.standard_normal(10)
    sb = body.SkinnedBody.from_smplx_npz(path, betas=betas, expression=expr, device=DEV)
    direct = body.SkinnedBody(b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"], shapedirs=shapedirs,
                              posedirs=b["posedirs"], betas=np.concatenate([betas, expr]), device=DEV)
    for name in ("v_shaped", "J_rest", "parents", "posedirs", "weight_joint", "weight_value", "faces"):
        assert torch.equal(getattr(sb, name), getattr(direct, name)), name
    b["shapedirs"] = shapedirs
    v_shaped, _ = lr.setup(b, np.concatenate([betas, expr]))
    assert np.array_equal(sb.v_shaped.cpu().numpy(), v_shaped.astype(np.float32))
    poses = lr.make_poses("random", 2, 55, seed=92)
    v = sb.pose(poses)
    assert torch.equal(v, direct.pose(poses))
    ids = [3, 69, 0, 41, 17]
    picked = body.SkinnedBody.extra_joints(v, ids)
    assert picked.shape == (2, 5, 3) and torch.equal(picked, v[:, ids])


# ----------------------------------------------------------------------------------------------------------- errors

def test_cpu_tensors_and_too_many_joints_raise():
    b = lr.make_body(20, 5, "chain", 2, True, seed=95)
    sb = body.SkinnedBody(b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"], posedirs=b["posedirs"], device=DEV)
    with pytest.raises(RuntimeError, match="HIP device"):
        sb.pose(torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        sb.pose(torch.zeros(5, 3, device=DEV), transl=torch.zeros(3))
    with pytest.raises(ValueError):
        sb.pose(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        sb.pose(np.zeros((2, 5, 3), np.float32), transl=np.zeros((3, 3), np.float32))
    with pytest.raises(RuntimeError, match="HIP device"):
        _lib.load_binding().lbs_pose(sb.v_shaped.cpu(), sb.J_rest.cpu(), sb.parents.cpu(), None, sb.weight_joint.cpu(),
                                     sb.weight_value.cpu(), torch.zeros(1, 5, 3))
    big = lr.make_body(20, 64, "chain", 2, False, seed=96)
    with pytest.raises(ValueError, match="joints"):
        body.SkinnedBody(big["v_template"], big["faces"], list(big["parents"]) + [63], np.zeros((65, 20), np.float32),
                         np.zeros((20, 65), np.float32), device=DEV)
    with pytest.raises(RuntimeError, match="joints"):                          # and the binding itself, handed 65 joints
        _lib.load_binding().lbs_pose(sb.v_shaped, torch.zeros(65, 3, device=DEV), torch.zeros(65, dtype=torch.int32, device=DEV),
                                     None, sb.weight_joint, sb.weight_value, torch.zeros(1, 65, 3, device=DEV))
    a = _lib.HgsLbsArgs()
    a.V, a.J, a.F, a.weight_width = 20, 65, 1, 1
    assert _lib.load().hgs_lbs_pose(a, None) == -1
    # an empty batch is an empty result, without a launch
    v, j = sb.pose(np.zeros((0, 5, 3), np.float32), return_joints=True)
    assert v.shape == (0, 20, 3) and j.shape == (0, 5, 3)
    torch.cuda.synchronize()
