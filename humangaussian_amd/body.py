"""A skinned body model (SMPL-X and its kin) posed on the device: `SkinnedBody.pose` is linear blend skinning in two HIP
launches (csrc/lbs.hip, include/hgs_rast.h: hgs_lbs_pose).

Reference: /root/reference/animation.py
  :273-330   `load_smplx`: per frame a full SMPL-X forward through the `smplx` package on the CPU, `.detach().cpu().numpy()`
             of the 10 475 vertices, then recentring and rescaling in numpy              -> `SkinnedBody.pose` (the affine
                                                                                            is the kernel's last step)
  :552-556   the frame loop calls it for every frame                                     -> `animation.SMPLXDriver`

[UPSTREAM-KNOWLEDGE] the `smplx` package is not part of the reference tree; what is restated here is its `lbs()`:
v_shaped = v_template + shapedirs . [betas, expression];  J = J_regressor . v_shaped;  pose feature = (R_j - I) of the
joints j >= 1;  v_posed = v_shaped + pose feature . posedirs;  the kinematic chain;  v = sum_j w_j (A_j v_posed).  The
set-up (once per body) runs in float64 on the host and is cast once; everything per frame runs on the device.  There is
no CPU path: poses on the CPU are uploaded, tensors handed to the constructor may live anywhere, a CPU `device` raises.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_JOINTS = _lib.LBS_MAX_JOINTS
FRAME_TILE = _lib.LBS_FRAME_TILE
# [UPSTREAM-KNOWLEDGE] kintree_table[0] of the SMPL-X model file: 22 body joints, jaw, two eyes, 2 x 15 finger joints
SMPLX_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53)


def _np(x, dtype=np.float64) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(dtype)


def check_parents(parents) -> np.ndarray:
    """parents[0] = -1 and 0 <= parents[j] < j: the order the kinematic chain relies on (the kernel trusts it)"""
    p = _np(parents, np.int64).reshape(-1)
    if p.size < 1 or p.size > MAX_JOINTS:
        raise ValueError(f"a body has 1..{MAX_JOINTS} joints, got {p.size}")
    if p[0] != -1 and p[0] != 0xffffffff:                  # (the model file stores the root's parent as uint32 -1)
        raise ValueError(f"parents[0] must be -1, got {p[0]}")
    for j in range(1, p.size):
        if not 0 <= p[j] < j:
            raise ValueError(f"parents is not in topological order: parents[{j}] = {p[j]}")
    p[0] = -1
    return p.astype(np.int32)


def pack_weights(weights):
    """Dense (V, J) skinning weights -> (joint (V, W) int32, value (V, W) fp32), W = the most non-zeros of any vertex (at
    least 1): a vertex's non-zero weights with their joints in ascending order, then slots (joint 0, weight 0).  Exact:
    `unpack_weights` gives the dense matrix back."""
    w = _np(weights, np.float32)
    if w.ndim != 2:
        raise ValueError("weights must be (V, J)")
    V, J = w.shape
    nz = w != 0
    W = max(1, int(nz.sum(1).max())) if V else 1
    order = np.argsort(~nz, axis=1, kind="stable")[:, :W]                 # non-zero columns first, ascending inside
    value = np.take_along_axis(w, order, 1)
    joint = np.where(value != 0, order, 0).astype(np.int32)
    return joint, np.ascontiguousarray(value, np.float32)


def unpack_weights(joint, value, J: int) -> np.ndarray:
    joint, value = _np(joint, np.int64), _np(value, np.float32)
    dense = np.zeros((joint.shape[0], J), np.float32)
    np.add.at(dense, (np.arange(joint.shape[0])[:, None], joint), value)  # (padding slots add 0 to joint 0)
    return dense


def pad_posedirs(posedirs, V: int) -> np.ndarray:
    """(K, 3 V) -> (K, 12 ceil(V / 4)) fp32, zero padded: every row starts on a 16-byte boundary and every thread of the
    skinning kernel loads whole 16-byte pieces of it (four vertices)"""
    pd = _np(posedirs, np.float32)
    out = np.zeros((pd.shape[0], 12 * ((V + 3) // 4)), np.float32)
    out[:, :3 * V] = pd
    return out


class SkinnedBody:
    """v_template (V, 3), faces (T, 3), parents (J,), J_regressor (J, V), weights (V, J) dense, shapedirs (V, 3, S) or None,
    posedirs None (no pose blend shapes), (9 (J - 1), 3 V) (the lbs layout) or (V, 3, 9 (J - 1)) (the model file's), betas
    (<= S,) or None: the coefficients of the first shape directions.  Everything `pose` needs stays on `device`."""

    def __init__(self, v_template, faces, parents, J_regressor, weights, shapedirs=None, posedirs=None, betas=None,
                 device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("humangaussian_amd: a SkinnedBody lives on a HIP device (there is no CPU path)")
        v = _np(v_template)
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
            raise ValueError("v_template must be (V, 3) with V >= 1")
        V = v.shape[0]
        par = check_parents(parents)
        J = par.size
        reg, w = _np(J_regressor), _np(weights, np.float32)
        if reg.shape != (J, V):
            raise ValueError(f"J_regressor must be ({J}, {V}), got {reg.shape}")
        if w.shape != (V, J):
            raise ValueError(f"weights must be ({V}, {J}), got {w.shape}")
        if betas is not None:
            b = _np(betas).reshape(-1)
            if shapedirs is None:
                raise ValueError("betas without shapedirs")
            sd = _np(shapedirs)
            if sd.ndim != 3 or sd.shape[:2] != (V, 3) or sd.shape[2] < b.size:
                raise ValueError(f"shapedirs must be ({V}, 3, S) with S >= {b.size}, got {sd.shape}")
            v = v + sd[:, :, :b.size] @ b
        K = 9 * (J - 1)
        pd = None
        if posedirs is not None and K > 0:
            pd = _np(posedirs, np.float32)
            if pd.shape == (V, 3, K):
                pd = np.ascontiguousarray(pd.reshape(3 * V, K).T)       # [UPSTREAM-KNOWLEDGE] smplx: posedirs.reshape(-1, K).T
            if pd.shape != (K, 3 * V):
                raise ValueError(f"posedirs must be ({K}, {3 * V}) or ({V}, 3, {K}), got {pd.shape}")
        faces = _np(faces, np.int64).reshape(-1, 3)
        if faces.size and (faces.min() < 0 or faces.max() >= V):
            raise ValueError("faces index outside the vertices")
        self.num_vertices, self.num_joints, self.num_pose_rows = V, J, (K if pd is not None else 0)
        self.parents_host = par
        self.v_shaped64, self.J_rest64 = v, reg @ v
        wj, wv = pack_weights(w)
        dev = self.device
        self.faces = torch.from_numpy(faces.astype(np.int32)).to(dev)
        self.v_shaped = torch.from_numpy(v.astype(np.float32)).to(dev)
        self.J_rest = torch.from_numpy(self.J_rest64.astype(np.float32)).to(dev)
        self.parents = torch.from_numpy(par).to(dev)
        self.weight_joint, self.weight_value = torch.from_numpy(wj).to(dev), torch.from_numpy(wv).to(dev)
        self.weight_width = wj.shape[1]
        self.posedirs = torch.from_numpy(pad_posedirs(pd, V)).to(dev) if pd is not None else None

    @classmethod
    def from_smplx_npz(cls, path, betas=None, expression=None, num_betas: int = 10, num_expression_coeffs: int = 10,
                       device="cuda") -> "SkinnedBody":
        """A body from the standard SMPL-X model file (`SMPLX_NEUTRAL.npz`: keys v_template, f, kintree_table, J_regressor,
        weights, shapedirs, posedirs).  [UPSTREAM-KNOWLEDGE] the layout of shapedirs: a 400-wide table holds 300 shape
        directions followed by 100 expression directions (expression starts at index 300); a 20-wide one (the 10 + 10 table
        of the older files) holds the expression directions from index `num_betas` on.  Any other width raises.
        betas (<= num_betas,) and expression (<= num_expression_coeffs,) default to zero.
        Only the reference's convention `flat_hand_mean=True, use_pca=False` (animation.py:292-303) is supported: hand poses
        are 15 axis-angle joints per hand, used as given - no PCA components, no mean hand pose added."""
        with np.load(path, allow_pickle=True) as f:
            missing = [k for k in ("v_template", "f", "kintree_table", "J_regressor", "weights", "shapedirs", "posedirs")
                       if k not in f]
            if missing:
                raise KeyError(f"{path}: not an SMPL-X model file, missing {missing}")
            data = {k: np.asarray(f[k]) for k in ("v_template", "f", "kintree_table", "J_regressor", "weights", "shapedirs",
                                                  "posedirs")}
        sd = data["shapedirs"].astype(np.float64)
        width = sd.shape[-1]
        if width == 400:
            expr_start = 300
        elif width == 20:
            expr_start = num_betas
        else:
            raise ValueError(f"{path}: shapedirs of width {width}: 400 (300 shape + 100 expression) or 20 expected")
        if num_betas > expr_start or expr_start + num_expression_coeffs > width:
            raise ValueError(f"num_betas {num_betas} / num_expression_coeffs {num_expression_coeffs} do not fit a table of "
                             f"width {width}")
        b = np.zeros(num_betas)
        e = np.zeros(num_expression_coeffs)
        if betas is not None:
            bb = _np(betas).reshape(-1)
            if bb.size > num_betas:
                raise ValueError(f"{bb.size} betas for num_betas = {num_betas}")
            b[:bb.size] = bb
        if expression is not None:
            ee = _np(expression).reshape(-1)
            if ee.size > num_expression_coeffs:
                raise ValueError(f"{ee.size} expression coefficients for num_expression_coeffs = {num_expression_coeffs}")
            e[:ee.size] = ee
        dirs = np.concatenate([sd[:, :, :num_betas], sd[:, :, expr_start:expr_start + num_expression_coeffs]], axis=2)
        return cls(data["v_template"], data["f"], data["kintree_table"][0], data["J_regressor"], data["weights"],
                   shapedirs=dirs, posedirs=data["posedirs"], betas=np.concatenate([b, e]), device=device)

    def _poses(self, poses) -> torch.Tensor:
        if not isinstance(poses, torch.Tensor):
            poses = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float32))).to(self.device)
        elif poses.device.type != "cuda":
            raise RuntimeError("humangaussian_amd: tensors must live on a HIP device (there is no CPU path)")
        p = poses.to(self.device, torch.float32)
        if p.dim() == 2:
            p = p[None]
        if p.dim() != 3 or tuple(p.shape[1:]) != (self.num_joints, 3):
            raise ValueError(f"poses must be ({self.num_joints}, 3) or (F, {self.num_joints}, 3), got {tuple(poses.shape)}")
        return p.contiguous()

    @torch.no_grad()
    def pose(self, poses, transl=None, centre=None, scale: float = 1.0, return_joints: bool = False):
        """poses (J, 3) or (F, J, 3) axis-angle (numpy or a device tensor; a CPU tensor raises) -> vertices (F, V, 3) on the
        device: ((lbs(pose) + transl) - centre) * scale.  transl (3,) or (F, 3), centre (3,).  return_joints=True: also the
        posed joints (F, J, 3) under the same affine.  Frame f of a batch has the bits of a call with that frame alone."""
        p = self._poses(poses)
        F = p.shape[0]
        t = None
        if transl is not None:
            if isinstance(transl, torch.Tensor) and transl.device.type != "cuda":
                raise RuntimeError("humangaussian_amd: tensors must live on a HIP device (there is no CPU path)")
            t = torch.as_tensor(transl, dtype=torch.float32).to(self.device, torch.float32).reshape(-1, 3)
            if t.shape[0] not in (1, F):
                raise ValueError(f"transl must be (3,) or ({F}, 3)")
            t = t.expand(F, 3).contiguous()
        c = [0.0, 0.0, 0.0] if centre is None else [float(x) for x in _np(centre).reshape(3)]
        verts, joints = _lib.load_binding().lbs_pose(self.v_shaped, self.J_rest, self.parents, self.posedirs, self.weight_joint,
                                                     self.weight_value, p, t, c, float(scale), bool(return_joints))
        return (verts, joints) if return_joints else verts

    @staticmethod
    def extra_joints(vertices: torch.Tensor, vertex_ids: Sequence[int]) -> torch.Tensor:
        """The joints the body model picks from its surface - the reference's nose, eyes and ears (entries 55-59 of
        `joint_mapper_smplx_to_openpose18`): (F, V, 3) vertices -> (F, len(vertex_ids), 3), a plain index."""
        idx = torch.as_tensor(list(vertex_ids), dtype=torch.long, device=vertices.device)
        return vertices.index_select(-2, idx)
