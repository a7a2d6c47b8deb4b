"""The animation path (BASELINE.json configs[4]): per frame re-anchor the avatar's Gaussians
on the posed body mesh, render forward-only, hand the frame to the consumer - frames sharded over the GPUs of a node.

Reference: /root/reference/animation.py
  :384-403   per frame: closest points + signed distance along the face normal -> new xyz, computed with numpy on the
             CPU and uploaded (`.cuda()` at :403)                      -> `MeshAnchoredGaussians.positions` (one HIP pass,
                                                                          the mapping stays resident: hgs_reanchor)
  :477-484   `render_gs`: MiniCam -> `Renderer.render` -> image `.detach().cpu()`   -> `AvatarAnimator.render_frame`
  :966-1004  the frame loop (azimuth i % 360, elevation 0, radius 2, fovy 50; pose i)  -> `render_frames_parallel`:
             frame i belongs to rank i mod G (frames are independent units: no data-path collective is NEEDED; the
             optional image all-gather, one per round of G frames, runs under the render of the next round)

Beyond the reference, opt-in and off by default: `AvatarAnimator(..., repose_rotations=True)` also carries every Gaussian's
rotation with its anchor face (`MeshAnchoredGaussians.bind_rotations` / `positions_and_rotations`: hgs_reanchor_rot).

The host logic (`render_frames_parallel`) takes the per-frame render as a callable, so it is testable on CPU with gloo; the
product pieces (`MeshAnchoredGaussians`, `AvatarAnimator`) run on the HIP rasterizer only - there is no CPU fallback.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Iterator, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .view_parallel import _Gather, shard_views


class MeshAnchoredGaussians:
    """Holds the static mapping (face index, barycentric uvw, signed distance along the face normal:
    animation.py:339-345) on the device; `positions(vertices)` -> (P,3) for a posed mesh.

    Opt-in, beyond the reference (which moves positions only): `bind_rotations(rest_vertices, rotation_raw)` once, then
    `positions_and_rotations(vertices)` -> ((P,3), (P,4)): every Gaussian's quaternion is carried by the rotation of its
    anchor face from the rest mesh to the posed mesh, in the pass that writes its position (include/hgs_rast.h:
    hgs_reanchor_rot; the face frame is e1 = first edge, n = face normal, e2 = n x e1).  The rotations returned are RAW
    (they keep the length of `rotation_raw`; `get_rotation` normalises as always).  Scales are not re-posed and colours do
    not rotate: with an active SH degree > 0 the view-dependent part stays in world axes."""

    def __init__(self, faces, mapping_face, mapping_uvw, mapping_dist, device="cuda"):
        dev = torch.device(device)
        self.faces = torch.as_tensor(faces).to(dev, torch.int32).contiguous()
        self.mapping_face = torch.as_tensor(mapping_face).to(dev, torch.int32).contiguous()
        self.mapping_uvw = torch.as_tensor(mapping_uvw).to(dev, torch.float32).contiguous()
        self.mapping_dist = torch.as_tensor(mapping_dist).to(dev, torch.float32).contiguous()
        self.rot_base = None

    def positions(self, vertices) -> torch.Tensor:
        v = torch.as_tensor(vertices).to(self.faces.device, torch.float32).contiguous()
        return _lib.load_binding().reanchor(v, self.faces, self.mapping_face, self.mapping_uvw, self.mapping_dist)

    def bind_rotations(self, rest_vertices, rotation_raw) -> torch.Tensor:
        """rot_base[i] = conj(r(rest face of i)) (x) rotation_raw[i], kept on the device (one launch, once per avatar).
        `rotation_raw`: (P,4) raw `_rotation` parameter, rows in the order of the mapping."""
        v = torch.as_tensor(rest_vertices).to(self.faces.device, torch.float32).contiguous()
        q = torch.as_tensor(rotation_raw).detach().to(self.faces.device, torch.float32).contiguous()
        if q.dim() != 2 or q.shape[1] != 4 or q.shape[0] != self.mapping_face.numel():
            raise ValueError(f"bind_rotations: rotation_raw must be ({self.mapping_face.numel()}, 4), got {tuple(q.shape)}")
        self.rot_base = _lib.load_binding().reanchor_rot(v, self.faces, self.mapping_face, self.mapping_uvw,
                                                         self.mapping_dist, q, True)[1]
        return self.rot_base

    def positions_and_rotations(self, vertices) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (xyz (P,3) with the bits of `positions(vertices)`, rot (P,4) = r(posed face of i) (x) rot_base[i]), one launch"""
        if self.rot_base is None:
            raise RuntimeError("MeshAnchoredGaussians.positions_and_rotations: call bind_rotations(rest_vertices, "
                               "rotation_raw) first - there is no rest-pose frame to carry the rotations from")
        v = torch.as_tensor(vertices).to(self.faces.device, torch.float32).contiguous()
        xyz, rot = _lib.load_binding().reanchor_rot(v, self.faces, self.mapping_face, self.mapping_uvw, self.mapping_dist,
                                                    self.rot_base, False)
        return xyz, rot


# ------------------------------------------------------------------------------ the motion that drives the frames

# toy skeleton on the body mesh (`synth.human_mesh()`: A-pose, z-up, left = +x): SMPL-X joint index,
# centre, and the smooth weight of the part that follows the joint.  Parents before children.
_JOINTS = (
    # name, SMPL-X joint, parent, centre (x, y, z)
    ("l_shoulder", 16, None, (0.20, 0.0, 0.50)), ("l_elbow", 18, "l_shoulder", (0.40, 0.0, 0.30)),
    ("r_shoulder", 17, None, (-0.20, 0.0, 0.50)), ("r_elbow", 19, "r_shoulder", (-0.40, 0.0, 0.30)),
    ("l_hip", 1, None, (0.08, 0.0, -0.05)), ("l_knee", 4, "l_hip", (0.10, -0.03, -0.40)),
    ("r_hip", 2, None, (-0.08, 0.0, -0.05)), ("r_knee", 5, "r_hip", (-0.10, -0.03, -0.40)),
    ("head", 15, None, (0.0, 0.0, 0.58)),
)


def _smooth(t):
    t = t.clamp(0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def _part_weights(v: torch.Tensor):
    x, z = v[:, 0], v[:, 2]
    left, right = _smooth(x / 0.03 * 0.5 + 0.5), _smooth(-x / 0.03 * 0.5 + 0.5)
    arm_l, arm_r = _smooth((x - 0.17) / 0.06), _smooth((-x - 0.17) / 0.06)
    return {
        "l_shoulder": arm_l, "l_elbow": _smooth((x - 0.37) / 0.06),
        "r_shoulder": arm_r, "r_elbow": _smooth((-x - 0.37) / 0.06),
        "l_hip": _smooth((-0.02 - z) / 0.08) * left * (1 - arm_l), "l_knee": _smooth((-0.38 - z) / 0.06) * left * (1 - arm_l),
        "r_hip": _smooth((-0.02 - z) / 0.08) * right * (1 - arm_r), "r_knee": _smooth((-0.38 - z) / 0.06) * right * (1 - arm_r),
        "head": _smooth((z - 0.56) / 0.05) * (1 - arm_l) * (1 - arm_r),
    }


def _rodrigues(a: np.ndarray) -> np.ndarray:
    th = float(np.linalg.norm(a))
    if th < 1e-12:
        return np.eye(3)
    k = a / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


class MotionDriver:
    """Posed body-mesh vertices per frame, DRIVEN BY the reference's demo motion `content/amass_test_17.npz` (136 frames
    of 55 SMPL-X joint rotations) where the LOCAL asset humangaussian_amd/data/amass_test_17_poses.npz exists (built from
    the reference tree by data/make_motion.py; AMASS data, not redistributed), by a clip of the caller (`poses_path`: an
    .npz with `poses` (F, 55, 3)), or by a procedural sway of the same nine joints with the same period (`self.source` says
    which).  The SMPL-X model files that turn poses into vertices are not in the reference tree, so the angles of nine
    joints (shoulders, elbows, hips, knees, head) articulate the body mesh through smooth part weights instead - a toy
    skinning that moves the surface the way the real sequence moves its body (amplitude `gain`), which is all the
    rasterize path sees of it: `xyz` changes every frame, nothing else does (animation.py:384-403).  Frame i uses pose
    i mod 136 (animation.py:311-330)."""

    def __init__(self, vertices, device="cuda", gain: float = 0.6, poses_path: Optional[str] = None):
        self.device = torch.device(device)
        self.rest = torch.as_tensor(vertices, dtype=torch.float32).to(self.device)
        self.weights = _part_weights(self.rest)
        from . import data
        path = poses_path or data.MOTION
        if poses_path and not os.path.exists(poses_path):
            raise FileNotFoundError(poses_path)
        self.poses = np.load(path)["poses"].astype(np.float64) if os.path.exists(path) else None
        self.source = ("procedural sway (no motion asset)" if self.poses is None else
                       (os.path.basename(poses_path) if poses_path else "content/amass_test_17.npz poses (local asset)"))
        self.gain = gain
        self.num_poses = 136 if self.poses is None else int(self.poses.shape[0])

    def _angles(self, i: int):
        if self.poses is not None:
            return self.poses[i % self.num_poses]
        ph = 2.0 * math.pi * (i % self.num_poses) / self.num_poses
        a = np.zeros((55, 3))
        for j, (_, sj, _, _) in enumerate(_JOINTS):
            a[sj] = 0.4 * np.array([math.sin(ph + j), math.cos(2 * ph + j), math.sin(3 * ph + 2 * j)])
        return a

    def vertices(self, i: int) -> torch.Tensor:
        ang = self._angles(i)
        rest_c = {n: np.asarray(ce, np.float64) for n, _, _, ce in _JOINTS}
        Rw, cw, pack = {}, {}, np.zeros((len(_JOINTS), 4, 3), np.float32)      # per joint: (R_applied^T - I) rows, centre
        for j, (name, sj, parent, _) in enumerate(_JOINTS):                     # (host: nine 3x3 products, one upload)
            a = ang[sj] * self.gain
            # SMPL-X is y-up, the mesh z-up (poser.py:349-352 swaps y and z: a reflection, so the axis flips sign)
            Rl = _rodrigues(np.array([-a[0], -a[2], -a[1]]))
            if parent is None:
                Rp, c = np.eye(3), rest_c[name]
            else:                                          # the child's centre and frame ride on the parent
                Rp = Rw[parent]
                c = cw[parent] + Rp @ (rest_c[name] - rest_c[parent])
            Ra = Rp @ Rl @ Rp.T                            # the joint's rotation, applied in the posed frame about c
            Rw[name], cw[name] = Rp @ Rl, c
            pack[j, :3], pack[j, 3] = Ra.T - np.eye(3), c
        pk = torch.from_numpy(pack).to(self.device, non_blocking=True)
        v = self.rest.clone()
        for j, (name, _, _, _) in enumerate(_JOINTS):
            v = v + self.weights[name][:, None] * ((v - pk[j, 3]) @ pk[j, :3])
        return v


class SMPLXDriver:
    """Posed body-mesh vertices per frame from the body model itself: `body` is a `body.SkinnedBody` (for the reference: the
    SMPL-X model file, `SkinnedBody.from_smplx_npz`), `poses` a clip (F, J, 3) of axis-angle joint rotations (AMASS: the
    `poses` of the .npz, reshaped to (F, 55, 3)).  The interface `AvatarAnimator` takes from `MotionDriver`: `vertices(i)`,
    `num_poses`, `source`; frame i uses pose i mod F.

    body_only=True is the reference (animation.py:216, :292-303): `poses[:, 1:22]` drive joints 1-21, global orientation,
    jaw, eyes and hands stay zero.  body_only=False uses every joint of the clip as given.
    The recentring of animation.py:321-330 is part of every call: centre = the middle of the ZERO-pose vertices' box,
    scale = 0.6 / its largest side, times 1.1 ** 10; both are fixed at construction (the reference fixes them at its first
    forward).  `vertices(i)` is one `body.pose` call, `precompute(frames)` one batched call."""

    def __init__(self, body, poses, body_only: bool = True, source: str = "SMPL-X clip"):
        self.body, self.body_only, self.source = body, bool(body_only), source
        self.device = body.device
        p = poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
        p = np.asarray(p, np.float32).reshape(p.shape[0], -1, 3)
        J = body.num_joints
        if p.shape[0] < 1 or p.shape[1] < min(J, 22 if body_only else J):
            raise ValueError(f"poses must be (F >= 1, {J}, 3), got {p.shape}")
        full = np.zeros((p.shape[0], J, 3), np.float32)
        if body_only:
            hi = min(22, J)
            full[:, 1:hi] = p[:, 1:hi]
        else:
            full[:] = p[:, :J]
        self.poses = torch.from_numpy(full).to(self.device)
        self.num_poses = int(full.shape[0])
        rest = body.pose(np.zeros((J, 3), np.float32))[0]
        vmin, vmax = rest.min(0).values.cpu().numpy().astype(np.float32), rest.max(0).values.cpu().numpy().astype(np.float32)
        self.centre = (vmax + vmin) / 2
        self.scale = float(0.6 / np.max(vmax - vmin)) * 1.1 ** 10

    def vertices(self, i: int) -> torch.Tensor:
        return self.body.pose(self.poses[i % self.num_poses], centre=self.centre, scale=self.scale)[0]

    def rest_vertices(self) -> torch.Tensor:
        """(V, 3): the zero pose under the driver's affine - the mesh a trained avatar is anchored on (animation.py:333-345)"""
        return self.body.pose(torch.zeros_like(self.poses[0]), centre=self.centre, scale=self.scale)[0]

    def precompute(self, frames: Sequence[int]) -> torch.Tensor:
        """(len(frames), V, 3): the frames of the list in ONE call; row k has the bits of `vertices(frames[k])`"""
        idx = torch.as_tensor([int(i) % self.num_poses for i in frames], dtype=torch.long, device=self.device)
        return self.body.pose(self.poses.index_select(0, idx), centre=self.centre, scale=self.scale)


def human_mesh_anchors(n: int, seed: int = 0, device="cuda", max_dist: float = 0.004):
    """The body mesh (`synth.human_mesh()`: the reference's human.obj where the local asset exists, the procedural capsule
    mesh otherwise) + n Gaussians anchored on it the way animation.py:339-345 anchors a trained avatar: a face, barycentric
    coordinates, a signed distance along the face normal (area-uniform faces, |dist| <= max_dist).
    Returns (vertices (V,3) float32 numpy, MeshAnchoredGaussians)."""
    from . import synth
    mv, mf, _ = synth.human_mesh()
    v, f = mv.astype(np.float64), mf
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    rng = np.random.default_rng(seed)
    tri = np.searchsorted(np.cumsum(area) / area.sum(), rng.uniform(0, 1, n), side="right").clip(0, len(f) - 1)
    r1, r2 = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 1, n)
    uvw = np.stack([1.0 - r1, r1 * (1.0 - r2), r1 * r2], 1).astype(np.float32)
    dist_ = rng.uniform(-max_dist, max_dist, n).astype(np.float32)
    return mv, MeshAnchoredGaussians(f, tri.astype(np.int32), uvw, dist_, device=device)


def anchor_to_mesh(points, vertices, faces, max_error: float = 0.01):
    """Anchor a trained avatar's Gaussians on its body mesh the way the reference does once per avatar
    (/root/reference/animation.py:337-371): a "raystab" signed-distance query (`mesh.MeshIndex`, the HIP stand-in for
    cubvh), the rebuild closest + dist * unit face normal at the rest pose (hgs_reanchor, the pass every frame runs),
    err = |rebuilt - points| and keep = ~(err > max_error), the reference's own culling test.  Rows of non-finite points
    (face -1) are never kept, and their rebuild does not index a face.
    Returns (MeshAnchoredGaussians of the KEPT rows, keep (P,) bool, err (P,) fp32), all on the points' device."""
    from .mesh import MeshIndex
    pts = torch.as_tensor(points)
    if pts.device.type != "cuda":
        raise RuntimeError("humangaussian_amd: points must live on a HIP device (there is no CPU path)")
    pts = pts.detach().to(torch.float32).reshape(-1, 3).contiguous()
    index = MeshIndex(vertices, faces, device=pts.device)
    dist_, face, uvw = index.signed_distance(pts, return_uvw=True, mode="raystab")
    found = face >= 0
    face32 = torch.where(found, face, torch.zeros_like(face)).to(torch.int32)
    rebuilt = _lib.load_binding().reanchor(index.vertices, index.faces, face32, uvw, torch.where(found, dist_, 0.0))
    err = torch.where(found, torch.linalg.vector_norm(rebuilt - pts, dim=-1), float("nan"))
    keep = ~(err > max_error) & found
    anchors = MeshAnchoredGaussians(index.faces, face32[keep], uvw[keep], dist_[keep], device=pts.device)
    return anchors, keep, err


# ------------------------------------------------------------------------------ one frame, and the sharded loop

class AvatarAnimator:
    """Re-anchor + render of ONE frame on this rank's GPU: `render_frame(vertices, camera)` -> image (3,H,W) in [0,1]
    (`Renderer.render`: gs_renderer.py:923-1028 incl. its clamp), no autograd graph, the frame never leaves the device
    unless the caller moves it.  `gaussians` is any object with the reference GaussianModel getters and a writable
    `_xyz` (animation.py:403 assigns `self.gs.gaussians._xyz`).  antialiasing=True renders every frame with the
    rasterizer's screen-space antialiasing filter (`Renderer.render(..., antialiasing=True)`): thin structures keep
    their coverage at resolutions and distances other than the training ones.

    repose_rotations=True (off by default; beyond the reference, which moves positions only and leaves every Gaussian's
    orientation that of the rest pose): the animator binds `gaussians._rotation` to the anchor faces of `rest_vertices`
    at construction (`MeshAnchoredGaussians.bind_rotations`), and `render_frame` then assigns `_xyz` AND `_rotation`, the
    quaternion of each Gaussian carried by the rotation of its anchor face from the rest mesh to the posed one - flat or
    elongated Gaussians stay in the surface when a limb swings.  What is NOT re-posed: scales; and colours do not rotate -
    with an active SH degree > 0 the view-dependent part stays in world axes (the reference's animation always renders
    with degree 0, animation.py:212, where there is nothing to rotate).  With the switch off `render_frame` is the
    reference's path, call for call, and `_rotation` is never touched."""

    def __init__(self, gaussians, anchors: MeshAnchoredGaussians, white_background: bool = True, device="cuda",
                 antialiasing: bool = False, repose_rotations: bool = False, rest_vertices=None):
        from .renderer import Renderer
        self.gaussians, self.anchors = gaussians, anchors
        self.renderer = Renderer(gaussians, white_background=white_background, device=device)
        self.antialiasing = bool(antialiasing)
        self.repose_rotations = bool(repose_rotations)
        if self.repose_rotations:
            if rest_vertices is None:
                raise ValueError("AvatarAnimator(repose_rotations=True) needs rest_vertices=: the mesh the avatar was anchored on")
            anchors.bind_rotations(rest_vertices, gaussians._rotation)

    @classmethod
    def from_rest_pose(cls, gaussians, vertices, faces, max_error: float = 0.01, **kw) -> "AvatarAnimator":
        """The animator of a trained avatar: `anchor_to_mesh(gaussians.get_xyz, vertices, faces, max_error)` on its rest-pose
        body mesh, then the culling of the reference (animation.py:365-371): the six tensors `_xyz`, `_features_dc`,
        `_features_rest`, `_opacity`, `_scaling` and `_rotation` keep only the anchored rows (in place on `gaussians`).
        `keep` and `anchor_error` stay on the returned animator; **kw go to the constructor.  repose_rotations=True binds
        the culled `_rotation` (so that rows match) on `vertices`, the mesh the avatar was just anchored on."""
        anchors, keep, err = anchor_to_mesh(gaussians.get_xyz.detach(), vertices, faces, max_error=max_error)
        for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            setattr(gaussians, name, getattr(gaussians, name)[keep])
        if kw.get("repose_rotations"):
            kw["rest_vertices"] = vertices
        anim = cls(gaussians, anchors, **kw)
        anim.keep, anim.anchor_error = keep, err
        return anim

    @torch.no_grad()
    def render_frame(self, vertices, camera) -> torch.Tensor:
        if self.repose_rotations:                                            # opt-in: positions and rotations in one pass
            self.gaussians._xyz, self.gaussians._rotation = self.anchors.positions_and_rotations(vertices)
            return self.renderer.render(camera, antialiasing=self.antialiasing)["image"]
        self.gaussians._xyz = self.anchors.positions(vertices)               # animation.py:384-403, on the device
        return self.renderer.render(camera, antialiasing=self.antialiasing)["image"]      # animation.py:477-482

    @torch.no_grad()
    def render_mesh_frame(self, vertices, camera) -> torch.Tensor:
        """The loop's `mesh` mode (animation.py:538-541, `render_mesh_normal` :558-601): the posed mesh shaded with its vertex
        normals over a white background, (H, W, 3) in [0, 1] on the device, through the camera of `render_frame` - the two
        views agree pixel for pixel (`mesh_view.mvp_from_camera`).  The `MeshView` of `anchors.faces` is built at the first
        call."""
        from .mesh_view import MeshView, mvp_from_camera
        v = torch.as_tensor(vertices).to(self.anchors.faces.device, torch.float32)
        view = getattr(self, "_mesh_view", None)
        if view is None or view.num_vertices != v.shape[-2]:
            view = self._mesh_view = MeshView(self.anchors.faces, v.shape[-2], device=self.anchors.faces.device)
        mvp = mvp_from_camera(camera).to(v.device)
        return view.render_normals(v, mvp, int(camera.image_height), int(camera.image_width))[0]


def orbit_frame_camera(i: int, H: int, W: int, radius: float = 2.0, fovy_deg: float = 50.0, device="cuda"):
    """Camera of frame i as the reference's save loop sets it: elevation 0, azimuth i mod 360, radius 2, fovy 50
    (animation.py:936-945 defaults, :993-1000).  Host-side matrices, one small upload (renderer.cameras_from_c2w)."""
    from . import synth
    from .renderer import cameras_from_c2w
    return cameras_from_c2w(synth.c2w_orbit(0.0, float(i % 360), radius)[None], math.radians(fovy_deg), H, W, device=device)[0]


def render_frames_parallel(frames: Sequence[int], render_frame_fn: Callable[[int], torch.Tensor], group=None,
                           gather: bool = True) -> Iterator[Tuple[int, torch.Tensor]]:
    """Frames of an animation sharded over the ranks of `group`: frame number k of the list belongs to rank k mod G
    (`view_parallel.shard_views`), every rank renders only its own with `render_frame_fn(frame) -> (C,H,W)` tensor.

    gather=True   yields (frame, image) for EVERY frame, in list order, on every rank: round j = the frames j*G .. j*G+G-1,
                  one per rank; the round's images travel in ONE asynchronous all-gather (RCCL's own stream; gloo in the
                  CPU tests) that runs while round j+1 is rendered - only the last round's collective is exposed;
    gather=False  yields only this rank's frames, in order, and uses no collective at all (each rank writes its own frames).
    Works without an initialised process group (one rank)."""
    frames = list(frames)
    on = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank(group) if on else 0
    world = dist.get_world_size(group) if on else 1
    if not gather or world == 1:
        for k in shard_views(len(frames), rank, world):
            yield frames[k], render_frame_fn(frames[k])
        return
    if len(frames) < world:
        # checked on EVERY rank before the first collective (the same frame list and world size everywhere): a rank
        # without any frame could not size its slab, and raising only there would leave the others inside the all-gather
        raise ValueError(f"render_frames_parallel(gather=True): {len(frames)} frames for {world} ranks - pass at least "
                         f"one frame per rank, or gather=False")
    rounds = (len(frames) + world - 1) // world
    pending, shape_like = None, None

    def drain(j, g):
        allimg = g.result()                                   # (world, C, H, W)
        for r in range(world):
            k = j * world + r
            if k < len(frames):
                yield frames[k], allimg[r]
    for j in range(rounds):
        k = j * world + rank
        if k < len(frames):
            img = render_frame_fn(frames[k]).contiguous()
            shape_like = img
        else:                                                 # ragged last round: a zero frame nobody yields
            img = torch.zeros_like(shape_like)                #  (len(frames) >= world: this rank rendered round 0)
        started = _Gather(img, group, async_op=True)
        if pending is not None:
            yield from drain(j - 1, pending)
        pending = started
    if pending is not None:
        yield from drain(rounds - 1, pending)
