"""CPU tests of the skinned body's host side (no GPU): the numpy restatement the GPU tests measure the kernels with
(tests/lbs_reference.py) against closed forms and against itself in float64, over every case of the GPU sweep; the weight
packing, the `parents` check and the model-file loader of humangaussian_amd/body.py; the two new exports of the C ABI and
their argument validation, which launches nothing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lbs_reference as lr
from humangaussian_amd import _lib, body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the chunk sizes of csrc/lbs.hip (tests/test_gpu_lbs.py holds the same table)
CASES = lr.sweep_cases(verts_per_thread=4, verts_per_wave=64, verts_per_workgroup=64, frame_tile=_lib.LBS_FRAME_TILE)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


# ---------------------------------------------------------------------------------------------- the reference is sound

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_pose_returns_v_shaped_exactly(dtype):
    b = lr.make_body(37, 55, "smplx", 4, True, seed=1)
    v_shaped, J_rest = lr.setup(b, betas=[0.3, -1.0, 0.5])
    v, j = lr.pose(v_shaped, J_rest, b["parents"], b["weights"], b["posedirs"], np.zeros((2, 55, 3)), dtype=dtype)
    assert not np.isnan(v).any()
    if dtype is np.float64:        # sum_j w_j v_shaped: off v_shaped only by what the fp32 weights' sum is off 1
        slack = np.abs(b["weights"].astype(np.float64).sum(1) - 1.0).max() + 8 * np.finfo(np.float64).eps
        assert np.abs(v - v_shaped[None]).max() <= slack * (np.abs(v_shaped).max() + 2 * np.abs(J_rest).max())
        assert np.abs(j - J_rest[None]).max() <= 64 * np.finfo(np.float64).eps * np.abs(J_rest).max()
    # rotations are the identity and the pose feature zero EXACTLY: with one-hot weights nothing rounds at all
    onehot = np.zeros_like(b["weights"])
    onehot[np.arange(37), b["weights"].argmax(1)] = 1.0
    v1, _ = lr.pose(v_shaped, J_rest, b["parents"], onehot, b["posedirs"], np.zeros((1, 55, 3)), dtype=dtype)
    want = v_shaped.astype(dtype)
    J_ = J_rest.astype(dtype)
    # A_j.t = J_j - (I J_j) accumulates the chain's roundings of the joint offsets: zero for the root
    root = onehot[:, 0] == 1
    assert np.array_equal(v1[0][root], want[root])
    assert np.abs(v1[0] - want).max() <= 64 * np.finfo(dtype).eps * np.abs(J_).max()
    R = lr.rodrigues(np.zeros((4, 3)), dtype)
    assert np.array_equal(R, np.broadcast_to(np.eye(3, dtype=dtype), (4, 3, 3)))


def test_root_rotation_without_pose_blend_is_a_rigid_motion():
    b = lr.make_body(50, 6, "smplx", 3, False, seed=2)
    v_shaped, J_rest = lr.setup(b)
    a = np.array([0.3, -1.1, 0.7])
    poses = np.zeros((1, 6, 3))
    poses[0, 0] = a
    v, j = lr.pose(v_shaped, J_rest, b["parents"], b["weights"], None, poses)
    Rm = _rot(a, np.linalg.norm(a))
    want = (v_shaped - J_rest[0]) @ Rm.T + J_rest[0]
    # (the package's formula perturbs the angle by ~1e-8: compare at 1e-7)
    assert np.abs(v[0] - want).max() < 1e-7
    assert np.abs(j[0] - ((J_rest - J_rest[0]) @ Rm.T + J_rest[0])).max() < 1e-7


def test_two_joint_chain_with_one_hot_weights_matches_the_hand_written_expression():
    rng = np.random.default_rng(3)
    v_shaped = rng.uniform(-1, 1, (8, 3))
    J_rest = np.array([[0.0, 0.1, 0.0], [0.0, 0.6, 0.1]])
    weights = np.zeros((8, 2))
    weights[:4, 0] = 1.0
    weights[4:, 1] = 1.0
    a0, a1 = np.array([0.0, 0.0, 0.9]), np.array([1.2, 0.0, 0.0])
    posedirs = rng.standard_normal((9, 24)) * 0.01
    v, j = lr.pose(v_shaped, J_rest, [-1, 0], weights, posedirs, np.stack([a0, a1])[None],
                   transl=np.array([[0.5, 0.0, -0.25]]), centre=np.array([0.1, 0.2, 0.3]), scale=2.0)
    R0, R1 = _rot(a0, 0.9), _rot(a1, 1.2)
    v_posed = v_shaped + ((R1 - np.eye(3)).reshape(-1) @ posedirs).reshape(8, 3)
    top = (v_posed[:4] - J_rest[0]) @ R0.T + J_rest[0]
    j1 = R0 @ (J_rest[1] - J_rest[0]) + J_rest[0]
    bottom = (v_posed[4:] - J_rest[1]) @ (R0 @ R1).T + j1
    want = (np.concatenate([top, bottom]) + [0.5, 0.0, -0.25] - [0.1, 0.2, 0.3]) * 2.0
    assert np.abs(v[0] - want).max() < 1e-7
    assert np.abs(j[0, 1] - (j1 + [0.5, 0.0, -0.25] - [0.1, 0.2, 0.3]) * 2.0).max() < 1e-7


def test_sweep_covers_every_value_the_kernels_branch_on():
    T = _lib.LBS_FRAME_TILE
    seen = lambda key: {c[key] for c in CASES}    # noqa: E731
    assert {1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257} <= seen("V")
    assert seen("J") == {1, 2, 55, 64} and seen("tree") == {"chain", "star", "smplx"}
    assert {1, 4, 5, 55, 64} <= seen("width") and seen("pose_blend") == {True, False}
    assert seen("F") == {1, 2, T, T + 1, 136} and seen("poses") == {"zero", "tiny", "random", "pi"}
    assert seen("transl") == {True, False} and seen("affine") == {True, False}
    assert len({c["id"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_fp32_restatement_stays_close_to_fp64_on_the_sweep(case):
    """the unit of the GPU gate is the fp32 form's own error: it has to be small for the gate to mean anything"""
    c = lr.build_case(case)
    assert np.isfinite(c["v64"]).all() and np.isfinite(c["j64"]).all()
    print(case["id"], "fp32 err / (eps32 max|v|):", c["ref_err"] / (lr.EPS32 * c["vmax"]))
    assert c["ref_err"] <= 64 * lr.EPS32 * c["vmax"]
    if case["poses"] == "pi":
        n = np.linalg.norm(c["poses"].astype(np.float64), axis=-1)
        assert (n == float(np.float32(np.pi))).sum() >= case["F"]
    if case["poses"] == "tiny":
        assert np.allclose(np.linalg.norm(c["poses"].astype(np.float64), axis=-1), 1e-6, rtol=1e-3)


# ------------------------------------------------------------------------------------------------------ the host side

@pytest.mark.parametrize("width", [1, 4, 5, "J"])
def test_weight_packing_round_trips_exactly(width):
    J = 55
    w = J if width == "J" else width
    b = lr.make_body(70, J, "smplx", w, False, seed=4)
    joint, value = body.pack_weights(b["weights"])
    assert joint.dtype == np.int32 and value.dtype == np.float32 and joint.shape == value.shape == (70, w)
    assert np.array_equal(body.unpack_weights(joint, value, J), b["weights"])
    assert (value[0] != 0).all()                                           # vertex 0 fills the width
    nz = value != 0
    assert ((np.diff(joint, axis=1) > 0) | ~nz[:, 1:]).all()               # joints ascending over the used slots
    assert (joint[~nz] == 0).all() and (value >= 0).all()                  # padding: joint 0, weight 0
    assert (np.diff(nz.astype(int), axis=1) <= 0).all()                    # used slots first
    assert np.abs(b["weights"].sum(1) - 1).max() < 1e-6 and (b["weights"] >= 0).all()


def test_parents_must_be_topological():
    assert np.array_equal(body.check_parents([-1, 0, 1, 1]), [-1, 0, 1, 1])
    assert body.check_parents(np.array([0xffffffff, 0, 0], np.uint32))[0] == -1     # the model file's uint32 root
    for bad in ([-1, 2, 0], [0, 0, 1], [-1, 0, 2], [-1, -1], [-1, 1]):
        with pytest.raises(ValueError):
            body.check_parents(bad)
    with pytest.raises(ValueError):
        body.check_parents([-1] + list(range(64)))                         # 65 joints
    with pytest.raises(ValueError):
        body.check_parents([])
    for tree in ("chain", "star", "smplx"):
        for J in (1, 2, 55, 64):
            body.check_parents(lr.parents_of(tree, J))


def test_pad_posedirs_layout():
    pd = np.arange(18 * 15, dtype=np.float32).reshape(18, 15)              # V = 5
    out = body.pad_posedirs(pd, 5)
    assert out.shape == (18, 24) and np.array_equal(out[:, :15], pd) and (out[:, 15:] == 0).all()
    assert body.pad_posedirs(np.zeros((9, 12), np.float32), 4).shape == (9, 12)


def _write_model(path, width, V=11, J=4, seed=5):
    rng = np.random.default_rng(seed)
    b = lr.make_body(V, J, "smplx", 3, True, seed=seed)
    K = 9 * (J - 1)
    posedirs_file = b["posedirs"].T.reshape(V, 3, K)                      # the file's layout: (V, 3, K)
    shapedirs = (rng.standard_normal((V, 3, width)) * 0.03).astype(np.float32)
    kintree = np.stack([b["parents"].astype(np.int64) % (1 << 32), np.arange(J)]).astype(np.uint32)
    np.savez(path, v_template=b["v_template"], f=b["faces"].astype(np.uint32), kintree_table=kintree,
             J_regressor=b["J_regressor"], weights=b["weights"], shapedirs=shapedirs, posedirs=posedirs_file)
    return b, shapedirs


class _Captured(Exception):
    pass


@pytest.mark.parametrize("width,expr_start", [(400, 300), (20, 10)])
def test_from_smplx_npz_reads_both_shapedirs_widths(tmp_path, monkeypatch, width, expr_start):
    """the loader's host work, observed at the constructor it ends in (which needs a device)"""
    path = os.path.join(tmp_path, "model.npz")
    b, shapedirs = _write_model(path, width)
    seen = {}

    def fake_init(self, v_template, faces, parents, J_regressor, weights, shapedirs=None, posedirs=None, betas=None,
                  device="cuda"):
        seen.update(v_template=v_template, faces=faces, parents=parents, J_regressor=J_regressor, weights=weights,
                    shapedirs=shapedirs, posedirs=posedirs, betas=betas, device=device)

    monkeypatch.setattr(body.SkinnedBody, "__init__", fake_init)
    betas, expr = np.array([0.5, -0.25]), np.array([1.0, 2.0, 3.0])
    body.SkinnedBody.from_smplx_npz(path, betas=betas, expression=expr)
    assert np.array_equal(seen["v_template"], b["v_template"]) and np.array_equal(seen["weights"], b["weights"])
    assert body.check_parents(seen["parents"]).tolist() == b["parents"].tolist()
    assert seen["shapedirs"].shape == (11, 3, 20) and seen["betas"].shape == (20,)
    assert np.array_equal(seen["shapedirs"][:, :, :10], shapedirs[:, :, :10].astype(np.float64))
    assert np.array_equal(seen["shapedirs"][:, :, 10:], shapedirs[:, :, expr_start:expr_start + 10].astype(np.float64))
    assert seen["betas"].tolist() == [0.5, -0.25] + [0.0] * 8 + [1.0, 2.0, 3.0] + [0.0] * 7
    assert seen["posedirs"].shape == (11, 3, 27)
    with pytest.raises(ValueError):
        body.SkinnedBody.from_smplx_npz(path, betas=np.zeros(11))


def test_from_smplx_npz_refuses_a_third_width_and_a_cpu_device(tmp_path):
    path = os.path.join(tmp_path, "model.npz")
    _write_model(path, 30)
    with pytest.raises(ValueError, match="width 30"):
        body.SkinnedBody.from_smplx_npz(path)
    np.savez(os.path.join(tmp_path, "other.npz"), v_template=np.zeros((3, 3)))
    with pytest.raises(KeyError):
        body.SkinnedBody.from_smplx_npz(os.path.join(tmp_path, "other.npz"))
    path20 = os.path.join(tmp_path, "model20.npz")
    _write_model(path20, 20)
    with pytest.raises(RuntimeError, match="HIP device"):
        body.SkinnedBody.from_smplx_npz(path20, device="cpu")


def test_constructor_validates_shapes_before_it_touches_a_device():
    b = lr.make_body(9, 3, "chain", 2, True, seed=6)
    args = (b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"])
    with pytest.raises(RuntimeError, match="HIP device"):
        body.SkinnedBody(*args, device="cpu")
    if torch.cuda.is_available():
        return                                    # (the remaining refusals are the same code with a device at hand)
    for bad in ((b["v_template"][:, :2],) + args[1:], args[:2] + ([-1, 2, 0],) + args[3:],
                args[:3] + (b["J_regressor"][:, :5],) + args[4:], args[:4] + (b["weights"][:, :2],)):
        with pytest.raises((ValueError, RuntimeError)):
            body.SkinnedBody(*bad, device="cuda")


# ------------------------------------------------------------------------------------------------------------ the ABI

def test_abi_exports_and_argument_validation_without_a_gpu():
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    assert re.search(r"^int hgs_lbs_pose\(const hgs_lbs_args\* args, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^size_t hgs_lbs_workspace_bytes\(int32_t J, int32_t F\);", hdr, flags=re.M)
    assert int(re.search(r"#define HGS_LBS_MAX_JOINTS (\d+)", hdr).group(1)) == _lib.LBS_MAX_JOINTS == 64
    assert int(re.search(r"#define HGS_LBS_FRAME_TILE (\d+)", hdr).group(1)) == _lib.LBS_FRAME_TILE
    assert "hgs_lbs_pose" in _lib.EXPORTS and "hgs_lbs_workspace_bytes" in _lib.EXPORTS
    _lib.build()
    lib = _lib.load()
    assert lib.hgs_abi_version() == 17 == _lib.ABI_VERSION
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "hgs_lbs_pose") and hasattr(raw, "hgs_lbs_workspace_bytes")
    # the struct of the header, field for field
    fields = re.search(r"typedef struct hgs_lbs_args \{(.*?)\} hgs_lbs_args;", hdr, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", fields)
    assert names == [f[0] for f in _lib.HgsLbsArgs._fields_]
    assert _lib.HgsLbsArgs.v_shaped.offset == 24 and _lib.HgsLbsArgs.centre.offset == 88
    assert _lib.HgsLbsArgs.workspace.offset == 104 and ctypes.sizeof(_lib.HgsLbsArgs) == 128

    # sizing: A [F][J][12] + joints [F][J][3] + pf [F][9 (J - 1)] floats, rounded up to 256 bytes
    assert lib.hgs_lbs_workspace_bytes(55, 1) == (4 * (15 * 55 + 9 * 54) + 255) // 256 * 256
    assert lib.hgs_lbs_workspace_bytes(64, 136) >= 136 * 4 * (15 * 64 + 9 * 63)
    assert lib.hgs_lbs_workspace_bytes(1, 0) == 0 and lib.hgs_lbs_workspace_bytes(1, 1) == 256
    assert lib.hgs_lbs_workspace_bytes(0, 1) == 0 and lib.hgs_lbs_workspace_bytes(65, 1) == 0 and lib.hgs_lbs_workspace_bytes(2, -1) == 0

    def call(**kw):
        """a call whose every pointer is non-NULL (never dereferenced: each variant below is refused, or has nothing to do)"""
        a = _lib.HgsLbsArgs()
        a.V, a.J, a.F, a.K, a.weight_width, a.posedirs_stride = 10, 4, 0, 27, 2, 36
        for name in ("v_shaped", "J_rest", "parents", "posedirs", "weight_joint", "weight_value", "poses", "workspace", "vertices"):
            setattr(a, name, 4096)
        a.scale = 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.hgs_lbs_pose(ctypes.byref(a), None)

    OK, EINVAL = 0, -1
    assert lib.hgs_lbs_pose(None, None) == EINVAL
    assert call() == OK                                                     # F = 0
    assert call(F=3, V=0) == OK                                             # V = 0
    assert call(J=0, K=0) == EINVAL and call(J=65, K=9 * 64) == EINVAL and call(J=-1) == EINVAL
    assert call(J=64, K=9 * 63, weight_width=64) == OK and call(J=1, K=0, weight_width=1) == OK
    assert call(V=-1) == EINVAL and call(F=-1) == EINVAL
    assert call(weight_width=0) == EINVAL and call(weight_width=5) == EINVAL and call(weight_width=4) == OK
    assert call(K=26) == EINVAL and call(K=0, posedirs=None) == OK
    # with frames and vertices to pose, every array that has elements must be there (refused before any launch)
    for name in ("v_shaped", "J_rest", "parents", "posedirs", "weight_joint", "weight_value", "poses", "workspace", "vertices"):
        assert call(F=2, **{name: None}) == EINVAL, name
    assert call(F=2, posedirs_stride=35) == EINVAL and call(F=2, posedirs_stride=32) == EINVAL   # 4 | stride >= 12 ceil(V / 4)
    assert call(F=2, posedirs=4100) == EINVAL                               # 16-byte alignment of the table
    _lib.build_binding()
    doc = _lib.load_binding().lbs_pose.__doc__
    for arg in ("v_shaped", "J_rest", "parents", "posedirs", "weight_joint", "weight_value", "poses", "transl", "centre",
                "scale", "return_joints"):
        assert arg in doc
    with pytest.raises(RuntimeError, match="HIP device"):
        z = torch.zeros(1, 2, 3)
        _lib.load_binding().lbs_pose(torch.zeros(4, 3), torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32), None,
                                     torch.zeros(4, 1, dtype=torch.int32), torch.ones(4, 1), z)


def test_driver_and_pose_refuse_cpu_tensors():
    from humangaussian_amd.animation import SMPLXDriver
    assert {"vertices", "precompute"} <= set(dir(SMPLXDriver))
    b = lr.make_body(9, 3, "chain", 2, True, seed=7)
    with pytest.raises(RuntimeError, match="HIP device"):
        body.SkinnedBody(b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"], device="cpu")
