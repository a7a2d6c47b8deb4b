"""Pose-control images on the device: `PoseSkeleton.draw_views` draws the skeleton maps of all B views of a training step
in one HIP launch (csrc/pose.hip, include/hgs_rast.h: hgs_pose_draw) and never waits on the host.

Reference: threestudio/utils/poser.py
  :8-49      `draw_humansd_skeleton` (cv2.line + end circles, seaborn's hls palette)        -> the HumanSD style
  :361-414   `Skeleton.draw` (cv2 discs, ellipse polygons blended with addWeighted)         -> the OpenPose style
  :416-459   `Skeleton.humansd_draw`                                                        -> `humansd_draw`
  :61-104    the SMPL-X joint mappers                                                       -> `keypoints_from_joints`
  :336-346   recentre, rescale, y/z swap of `load_smplx`                                    -> `PoseSkeleton.from_body`
and threestudio/systems/GaussianDreamer.py:268-287, the per-view loop (mvp to the host, cv2 on the CPU, upload) that
`draw_views` replaces.  What is drawn is defined in include/hgs_rast.h (exact integer capsules, discs and ellipses); it is
not cv2 pixel for pixel - outline pixels may differ, and a keypoint that lands beyond +-8191 pixels (w <= 0) drops its
limbs where the reference would raise or let cv2 clip.

The tables below are written out from their public definitions: the COCO-17 keypoints and the skeleton MMPose / HumanSD
draw on them, the 18-point OpenPose body model with the controlnet_aux colour list, the SMPL-X joint names of the `smplx`
package ([UPSTREAM-KNOWLEDGE]: joint_names.py; 55-59 are the nose, eyes and ears it reads off the surface).  There is no
built-in default pose and no CPU path: tensors on the CPU raise.
"""
from __future__ import annotations

import colorsys
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

OPENPOSE, HUMANSD = _lib.POSE_OPENPOSE, _lib.POSE_HUMANSD
MAX_DIM = _lib.POSE_MAX_DIM

# COCO-17 keypoint order
HUMANSD_NAMES = ("nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow",
                 "right_elbow", "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle",
                 "right_ankle")
# OpenPose's 18-point body model
OPENPOSE_NAMES = ("nose", "neck", "right_shoulder", "right_elbow", "right_wrist", "left_shoulder", "left_elbow", "left_wrist",
                  "right_hip", "right_knee", "right_ankle", "left_hip", "left_knee", "left_ankle", "right_eye", "left_eye",
                  "right_ear", "left_ear")


def _pairs(names, pairs):
    return tuple((names.index(a), names.index(b)) for a, b in pairs)


# the COCO skeleton in HumanSD's drawing order; limb i is drawn in colour HUMANSD_LIMB_COLOUR[i] of the palette
HUMANSD_LINES = _pairs(HUMANSD_NAMES, (
    ("nose", "left_eye"), ("nose", "right_eye"), ("left_eye", "left_ear"), ("right_eye", "right_ear"),
    ("left_ear", "left_shoulder"), ("right_ear", "right_shoulder"), ("left_shoulder", "left_elbow"),
    ("right_shoulder", "right_elbow"), ("left_elbow", "left_wrist"), ("right_elbow", "right_wrist"),
    ("left_shoulder", "left_hip"), ("right_shoulder", "right_hip"), ("left_hip", "left_knee"), ("right_hip", "right_knee"),
    ("left_knee", "left_ankle"), ("right_knee", "right_ankle")))
HUMANSD_LIMB_COLOUR = tuple(i ^ 1 for i in range(16))          # left and right limbs swap the colours of a pair
HUMANSD_LIMBS = tuple((c, a, b) for c, (a, b) in zip(HUMANSD_LIMB_COLOUR, HUMANSD_LINES))
# the OpenPose limbs; limb i is drawn in colour i
OPENPOSE_LINES = _pairs(OPENPOSE_NAMES, (
    ("nose", "neck"), ("neck", "right_shoulder"), ("right_shoulder", "right_elbow"), ("right_elbow", "right_wrist"),
    ("neck", "left_shoulder"), ("left_shoulder", "left_elbow"), ("left_elbow", "left_wrist"), ("neck", "right_hip"),
    ("right_hip", "right_knee"), ("right_knee", "right_ankle"), ("neck", "left_hip"), ("left_hip", "left_knee"),
    ("left_knee", "left_ankle"), ("nose", "right_eye"), ("right_eye", "right_ear"), ("nose", "left_eye"),
    ("left_eye", "left_ear")))
OPENPOSE_LIMBS = tuple((i, a, b) for i, (a, b) in enumerate(OPENPOSE_LINES))
# controlnet_aux (open_pose/util.py): a hue wheel in steps of 85
OPENPOSE_COLOURS = ((255, 0, 0), (255, 85, 0), (255, 170, 0), (255, 255, 0), (170, 255, 0), (85, 255, 0), (0, 255, 0),
                    (0, 255, 85), (0, 255, 170), (0, 255, 255), (0, 170, 255), (0, 85, 255), (0, 0, 255), (85, 0, 255),
                    (170, 0, 255), (255, 0, 255), (255, 0, 170), (255, 0, 85))


def hls_palette(n: int = 16):
    """[UPSTREAM-KNOWLEDGE] seaborn.color_palette("hls", n) = hls_palette(n, h=.01, l=.6, s=.65): hues
    linspace(0, 1, n + 1)[:-1] + 0.01 through colorsys.hls_to_rgb; the reference takes int(255 c) of each channel."""
    hues = np.linspace(0, 1, n + 1)[:-1] + 0.01
    hues %= 1
    return tuple(tuple(int(255 * c) for c in colorsys.hls_to_rgb(float(h), 0.6, 0.65)) for h in hues)


# hls_palette(16), as the library holds it (tests/test_pose_image_cpu.py compares the two)
HUMANSD_COLOURS = ((219, 94, 86), (219, 144, 86), (219, 194, 86), (194, 219, 86), (145, 219, 86), (95, 219, 86),
                   (86, 219, 127), (86, 219, 177), (86, 211, 219), (86, 161, 219), (86, 111, 219), (111, 86, 219),
                   (160, 86, 219), (210, 86, 219), (219, 86, 178), (219, 86, 128))

# [UPSTREAM-KNOWLEDGE] the `smplx` package's joint names: the joints the two layouts use
SMPLX_JOINT = {"left_hip": 1, "right_hip": 2, "left_knee": 4, "right_knee": 5, "left_ankle": 7, "right_ankle": 8, "neck": 12,
               "left_shoulder": 16, "right_shoulder": 17, "left_elbow": 18, "right_elbow": 19, "left_wrist": 20,
               "right_wrist": 21, "nose": 55, "right_eye": 56, "left_eye": 57, "right_ear": 58, "left_ear": 59}
SMPLX_TO_HUMANSD17 = tuple(SMPLX_JOINT[n] for n in HUMANSD_NAMES)
SMPLX_TO_OPENPOSE18 = tuple(SMPLX_JOINT[n] for n in OPENPOSE_NAMES)


def _style(style) -> int:
    """'openpose' / 'humansd', the library's constants, or the reference's `humansd_style` flag"""
    if isinstance(style, str):
        if style in ("openpose", "humansd"):
            return HUMANSD if style == "humansd" else OPENPOSE
    elif isinstance(style, (bool, np.bool_)):
        return HUMANSD if style else OPENPOSE
    elif style in (OPENPOSE, HUMANSD):
        return int(style)
    raise ValueError(f"style is 'openpose' or 'humansd', got {style!r}")


def keypoints_from_joints(joints, style):
    """SMPL-X joints (..., >= 60, 3) - the 55 posed joints followed by nose, right eye, left eye, right ear, left ear
    (`SkinnedBody.extra_joints`) - in the order of the 17-point ('humansd') or 18-point ('openpose') layout.  numpy in,
    numpy out; a tensor stays where it is."""
    idx = SMPLX_TO_HUMANSD17 if _style(style) == HUMANSD else SMPLX_TO_OPENPOSE18
    if joints.shape[-2] < 60:
        raise ValueError(f"joints must cover indices 0..59 (55 joints + nose, eyes, ears), got {joints.shape[-2]}")
    if isinstance(joints, torch.Tensor):
        return joints.index_select(-2, torch.as_tensor(idx, dtype=torch.long, device=joints.device))
    return np.asarray(joints)[..., list(idx), :]


def default_limb_width(H: int) -> int:
    """the reference's humansd_skeleton_width: int(10 H / 512)"""
    return int(10 * H / 512)


def _no_cpu(t):
    if isinstance(t, torch.Tensor) and t.device.type != "cuda":
        raise RuntimeError("humangaussian_amd: tensors must live on a HIP device (there is no CPU path)")


class PoseSkeleton:
    """The parts of the reference's `Skeleton` a training step uses.  points3D (K, 3) or (K, 4), numpy or a device tensor,
    K = 17 (humansd_style) or 18, in the convention of the reference's `Skeleton.points3D`: y and z already swapped
    (`from_body` does that for SMPL-X joints); a fourth column is used as given, else it is 1."""

    def __init__(self, points3D, humansd_style: bool = False, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("humangaussian_amd: a PoseSkeleton lives on a HIP device (there is no CPU path)")
        _no_cpu(points3D)
        self.style = "humansd" if humansd_style else "openpose"
        self.name = list(HUMANSD_NAMES if humansd_style else OPENPOSE_NAMES)
        K = len(self.name)
        if isinstance(points3D, torch.Tensor):
            p = points3D.detach().to(self.device, torch.float32)
        else:
            p = torch.from_numpy(np.ascontiguousarray(np.asarray(points3D, dtype=np.float32))).to(self.device)
        if p.dim() != 2 or p.shape[0] != K or p.shape[1] not in (3, 4):
            raise ValueError(f"points3D must be ({K}, 3) or ({K}, 4) for the {self.style} style, got {tuple(p.shape)}")
        if p.shape[1] == 3:
            p = torch.cat([p, torch.ones_like(p[:, :1])], dim=1)
        self.points3D = p.contiguous()

    @classmethod
    def from_joints(cls, joints, humansd_style: bool = False, device="cuda") -> "PoseSkeleton":
        """SMPL-X joints (>= 60, 3) in the body model's axes (see `keypoints_from_joints`) -> the skeleton: the layout's
        keypoints with y and z swapped (poser.py:345)."""
        kp = keypoints_from_joints(joints, "humansd" if humansd_style else "openpose")
        kp = kp[..., [0, 2, 1]]
        return cls(kp, humansd_style=humansd_style, device=device)

    @classmethod
    def from_body(cls, body, poses, extra_vertex_ids: Sequence[int], humansd_style: bool = False):
        """The reference's `load_smplx` (poser.py:316-346) on a `SkinnedBody`: pose the body once to find the box of its
        vertices (one host read, at set-up), then `body.pose(poses, centre=(max + min) / 2, scale=0.6 / largest side,
        return_joints=True)`; the 55 joints and the surface joints `extra_vertex_ids` (nose, right eye, left eye, right
        ear, left ear) become the keypoints, y and z swapped.  poses: (J, 3).  Returns (skeleton, centre, scale)."""
        v = body.pose(poses)[0]
        vmin, vmax = v.min(0).values.cpu().numpy().astype(np.float64), v.max(0).values.cpu().numpy().astype(np.float64)
        centre, scale = (vmax + vmin) / 2, 0.6 / float(np.max(vmax - vmin))
        v, j = body.pose(poses, centre=centre, scale=scale, return_joints=True)
        joints = torch.cat([j[0], body.extra_joints(v[0], extra_vertex_ids)], dim=0)
        return cls.from_joints(joints, humansd_style=humansd_style, device=body.device), centre, scale

    @property
    def hand_centers(self) -> torch.Tensor:
        """(2, 3): the left and the right wrist, on the device"""
        return self.points3D[[self.name.index("left_wrist"), self.name.index("right_wrist")], :3]

    def _mvp(self, mvp) -> torch.Tensor:
        _no_cpu(mvp)
        if not isinstance(mvp, torch.Tensor):
            mvp = torch.from_numpy(np.ascontiguousarray(np.asarray(mvp, dtype=np.float32))).to(self.device)
        m = mvp.detach().to(self.device, torch.float32)
        if m.dim() == 2:
            m = m[None]
        if m.dim() != 3 or tuple(m.shape[1:]) != (4, 4):
            raise ValueError(f"mvp must be (4, 4) or (B, 4, 4), got {tuple(mvp.shape)}")
        return m.contiguous()

    @torch.no_grad()
    def draw_views(self, mvp, H: int, W: int, enable_occlusion=False, limb_width: Optional[int] = None,
                   dtype=torch.float32, return_records: bool = False):
        """mvp (B, 4, 4) (a device tensor or numpy; a CPU tensor raises) -> (images (B, H, W, 3), kp (B, K, 3): xs, ys,
        conf), one launch, nothing read back.  enable_occlusion: one bool for every view or (B,) bools.  limb_width: the
        HumanSD line width, default the reference's int(10 H / 512); below 1 raises (H < 52 needs an explicit width).
        dtype: torch.float32 (values v / 255) or torch.uint8 (v).  return_records=True: also the (B, R, 8) int32 records
        the raster read (include/hgs_rast.h)."""
        m = self._mvp(mvp)
        B = m.shape[0]
        H, W = int(H), int(W)
        if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
            raise ValueError(f"H and W must be in [1, {MAX_DIM}], got {H} x {W}")
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError("dtype is torch.float32 or torch.uint8")
        humansd = self.style == "humansd"
        if limb_width is None:
            limb_width = default_limb_width(H) if humansd else 1
        limb_width = int(limb_width)
        if limb_width < 1:
            raise ValueError(f"limb_width must be at least 1, got {limb_width} (the default int(10 H / 512) is 0 below H = 52)")
        occ = None
        if isinstance(enable_occlusion, (bool, np.bool_)):
            if enable_occlusion:
                occ = torch.ones(B, dtype=torch.uint8, device=self.device)
        else:
            _no_cpu(enable_occlusion)
            if isinstance(enable_occlusion, torch.Tensor):
                occ = (enable_occlusion.to(self.device) != 0).to(torch.uint8).reshape(-1).contiguous()
            else:
                occ = torch.from_numpy(np.ascontiguousarray(np.asarray(enable_occlusion).astype(bool).astype(np.uint8))
                                       ).reshape(-1).to(self.device)
            if occ.numel() != B:
                raise ValueError(f"enable_occlusion must be a bool or ({B},) bools")
        image, kp, records = _lib.load_binding().pose_draw(self.points3D, m, occ, HUMANSD if humansd else OPENPOSE, H, W,
                                                           limb_width, dtype == torch.uint8)
        return (image, kp, records) if return_records else (image, kp)

    def draw(self, mvp, H: int, W: int, enable_occlusion: bool = False):
        """the reference's `Skeleton.draw` for one view: (canvas (H, W, 3) fp32 in [0, 1], (18, 2) xs, ys), on the device"""
        if self.style != "openpose":
            raise ValueError("draw is the OpenPose style's; this skeleton has the 17 HumanSD keypoints (humansd_draw)")
        image, kp = self.draw_views(self._one(mvp), H, W, enable_occlusion=bool(enable_occlusion))
        return image[0], kp[0, :, :2]

    def humansd_draw(self, mvp, H: int, W: int, enable_occlusion: bool = False):
        """the reference's `Skeleton.humansd_draw` for one view: (image (H, W, 3) fp32 in [0, 1], kp (1, 17, 3)), on the
        device"""
        if self.style != "humansd":
            raise ValueError("humansd_draw is the HumanSD style's; this skeleton has the 18 OpenPose keypoints (draw)")
        image, kp = self.draw_views(self._one(mvp), H, W, enable_occlusion=bool(enable_occlusion))
        return image[0], kp

    def _one(self, mvp):
        m = self._mvp(mvp)
        if m.shape[0] != 1:
            raise ValueError("one view: mvp must be (4, 4)")
        return m
