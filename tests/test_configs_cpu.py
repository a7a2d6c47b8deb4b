"""BASELINE.json configs[0]: '~10k Gaussians PLY, single 512^2 view, PyTorch-CPU reference
render path (plumbing, no GPU)'.  content/sample.ply is missing from the reference mount
(.MISSING_LARGE_BLOBS), so a synthetic stand-in goes through the reference's PLY schema
(scene/gaussian_model.py:187-266) and the CPU oracle."""
import math
import os

import numpy as np
import pytest
import torch

import oracle
from humangaussian_amd import ply_io, synth


def test_ply_roundtrip_is_byte_stable_and_schema_matches_reference(tmp_path):
    cl = synth.init_cloud(500, 2, "mid", seed=3)
    raw = dict(xyz=cl.means3D.numpy(), features_dc=cl.shs[:, :1].numpy(), features_rest=cl.shs[:, 1:].numpy(),
               opacity=torch.logit(cl.opacities).numpy(), scaling=torch.log(cl.scales).numpy(),
               rotation=cl.rotations.numpy())
    p1, p2 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    ply_io.save_ply(p1, **raw)
    got = ply_io.load_ply(p1, max_sh_degree=2)
    for k, v in raw.items():
        assert np.array_equal(got[k], np.asarray(v, np.float32).reshape(got[k].shape)), k
    ply_io.save_ply(p2, **{k: got[k] for k in raw})
    assert open(p1, "rb").read() == open(p2, "rb").read()
    head = open(p1, "rb").read(2000).split(b"end_header\n")[0].decode().splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 500"]
    props = [ln.split()[2] for ln in head if ln.startswith("property float")]
    assert props == ply_io.attribute_names(3 * 9 - 3) and len(props) == 6 + 3 + 24 + 1 + 3 + 4
    # channel-major SH layout: f_rest_0..7 are the 8 non-DC coefficients of channel 0
    rows = np.frombuffer(open(p1, "rb").read().split(b"end_header\n", 1)[1], "<f4").reshape(500, -1)
    assert np.array_equal(rows[:, 9:17], raw["features_rest"][:, :, 0])


def test_config1_ply_to_cpu_render_512(tmp_path):
    P = 10_000
    cl = synth.init_cloud(P, 0, "mid", seed=0)
    path = str(tmp_path / "sample.ply")
    ply_io.save_ply(path, cl.means3D.numpy(), cl.shs[:, :1].numpy(), cl.shs[:, 1:].numpy(),
                    torch.logit(cl.opacities).numpy(), torch.log(cl.scales).numpy(), cl.rotations.numpy())
    g = ply_io.load_ply(path, max_sh_degree=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    xyz, shs = t(g["xyz"]), torch.cat([t(g["features_dc"]), t(g["features_rest"])], 1)
    opac, scales = torch.sigmoid(t(g["opacity"])), torch.exp(t(g["scaling"]))
    rots = torch.nn.functional.normalize(t(g["rotation"]))
    cam = synth.orbit_camera(15.0, 30.0, 2.0, 70.0, 512, 512)          # uncond.py eval defaults
    st = oracle.OracleSettings(512, 512, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.zeros(3), 1.0,
                               cam.world_view_transform, cam.full_proj_transform, 0, cam.camera_center, False, False)
    with torch.no_grad():
        c, r, d, a = oracle.rasterize(xyz, None, shs, None, opac, scales, rots, None, st)
    assert c.shape == (3, 512, 512) and r.dtype == torch.int32
    assert int((r > 0).sum()) > 0.95 * P                 # the whole body is in view
    cover = (a[0] > 0.5).float().mean().item()
    assert 0.02 < cover < 0.5                            # a person in the middle of the frame
    ys, xs = torch.nonzero(a[0] > 0.5, as_tuple=True)
    assert float(ys.max() - ys.min()) > float(xs.max() - xs.min())    # standing upright (taller than wide)... 


def test_renderer_python_sh_matches_reference_goldens():
    """renderer._eval_sh_python (the convert_SHs_python branch, degrees 0-3) against the outputs of
    the reference's own eval_sh (tests/golden/reference_helpers.npz, utils/sh_utils.py:57-112)."""
    import os
    import numpy as np
    from humangaussian_amd.renderer import _eval_sh_python
    ref = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_helpers.npz"))
    sh = torch.from_numpy(ref["sh_coeffs"]).double().transpose(1, 2)      # (P, 3, K) as the reference passes it
    d = torch.from_numpy(ref["sh_dirs"]).double()
    for deg in range(4):
        got = _eval_sh_python(deg, sh, d)
        assert np.abs(got.numpy() - ref[f"sh_eval_deg{deg}"]).max() < 2e-6, deg


def test_load_ply_kiui_axes_fixups_match_gs_renderer(tmp_path):
    """ply_io.load_ply(kiui_axes=True) == the fix-ups of the animation-side loader
    (/root/reference/gs_renderer.py:576-581) applied to the plain load."""
    import numpy as np
    from humangaussian_amd import ply_io
    rng = np.random.default_rng(4)
    P = 50
    xyz, dc, rest = rng.normal(size=(P, 3)), rng.normal(size=(P, 1, 3)), rng.normal(size=(P, 3, 3))
    op, sc, rot = rng.normal(size=(P, 1)), rng.normal(size=(P, 3)), rng.normal(size=(P, 4))
    path = tmp_path / "a.ply"
    ply_io.save_ply(path, xyz, dc, rest, op, sc, rot)
    plain = ply_io.load_ply(path)
    fixed = ply_io.load_ply(path, kiui_axes=True)
    # the reference's four lines, verbatim semantics
    xyz_r, scales_r, rots_r = plain["xyz"].copy(), plain["scaling"].copy(), plain["rotation"].copy()
    xyz_r[:, [1, 2]] = xyz_r[:, [2, 1]]
    scales_r[:, [1, 2]] = scales_r[:, [2, 1]]
    rots_r[:, [2, 3]] = rots_r[:, [3, 2]]
    rots_r[:, [0]] *= -1
    assert np.array_equal(fixed["xyz"], xyz_r) and np.array_equal(fixed["scaling"], scales_r)
    assert np.array_equal(fixed["rotation"], rots_r)
    for k in ("features_dc", "features_rest", "opacity"):
        assert np.array_equal(fixed[k], plain[k])
    assert not np.array_equal(fixed["xyz"], plain["xyz"])


def test_cameras_from_c2w_match_the_per_camera_arithmetic_and_append_rows():
    """renderer.cameras_from_c2w (host-side matrices of a whole step, one upload) == synth.camera_from_c2w per view
    (which tests/golden/reference_helpers.npz pins to the reference Camera class); densify.append_rows == the
    reference's cat_tensors_to_optimizer semantics (gaussian_model.py:339-357)."""
    import numpy as np
    import torch
    from humangaussian_amd import densify, renderer, synth
    c2ws = np.stack([synth.c2w_orbit(10.0 + 3 * i, 40.0 * i, 1.5 + 0.1 * i) for i in range(5)])
    fovy = np.radians([40.0, 50.0, 55.0, 60.0, 70.0])
    cams = renderer.cameras_from_c2w(c2ws, fovy, 96, 128, device="cpu")
    for i, c in enumerate(cams):
        ref = synth.camera_from_c2w(c2ws[i], float(fovy[i]), 96, 128)
        assert abs(c.FoVx - ref.FoVx) < 1e-12 and abs(c.FoVy - ref.FoVy) < 1e-12
        assert torch.equal(c.world_view_transform, ref.world_view_transform)
        assert torch.equal(c.full_proj_transform, ref.full_proj_transform)
        assert torch.equal(c.camera_center, ref.camera_center)
        assert (c.image_height, c.image_width) == (96, 128)
    xyz, m1 = torch.arange(12.0).reshape(4, 3), torch.ones(4, 3)
    acc = torch.arange(4.0).reshape(4, 1)
    new = torch.full((2, 3), 7.0)
    a, b, c_ = densify.append_rows([xyz, m1, acc], [new, None, None])
    assert torch.equal(a, torch.cat((xyz, new))) and torch.equal(b, torch.cat((m1, torch.zeros(2, 3))))
    assert torch.equal(c_, torch.cat((acc, torch.zeros(2, 1))))


@pytest.fixture()
def stand_in_assets(tmp_path, monkeypatch):
    """The two local assets of humangaussian_amd/data in their own formats, written from procedural stand-ins (the
    real ones - the reference's human.obj and its AMASS clip - are third-party data and never part of the repository):
    the capsule body mesh as human_mesh.npz, and a seeded 136-frame clip as amass_test_17_poses.npz that swings the nine
    driven joints with its own phases and amplitudes."""
    from humangaussian_amd import animation as an, data
    v, f = synth.humanoid_mesh()
    np.savez_compressed(tmp_path / "human_mesh.npz", vertices=v, faces=f, source="stand-in: synth.humanoid_mesh()")
    rng = np.random.default_rng(17)
    ph = 2 * np.pi * np.arange(136) / 136
    poses = rng.normal(0.0, 0.05, (136, 55, 3))
    for _, sj, _, _ in an._JOINTS:
        k, phase, amp = rng.integers(1, 3, 3), rng.uniform(0, 2 * np.pi, 3), rng.uniform(0.2, 0.6, 3)
        poses[:, sj] = amp * np.sin(k * ph[:, None] + phase)
    np.savez_compressed(tmp_path / "amass_test_17_poses.npz", poses=poses.astype(np.float32))
    monkeypatch.setattr(data, "HUMAN_MESH", str(tmp_path / "human_mesh.npz"))
    monkeypatch.setattr(data, "MOTION", str(tmp_path / "amass_test_17_poses.npz"))
    return data


def test_mesh_asset_cloud_is_seeded_area_uniform_and_on_the_asset_surface(stand_in_assets):
    """benchmark clouds are area-uniform samples of the local body-mesh asset
    (humangaussian_amd/data/human_mesh.npz: the reference's load/shapes/human.obj, normalised; built where the reference
    tree exists, not redistributed).  With a stand-in asset in the same format: `auto` resolves to it, the sampler is
    seeded and area-proportional and every point lies on the asset's surface."""
    data = stand_in_assets
    assert data.have_human_mesh()
    m = np.load(data.HUMAN_MESH)
    v, f = m["vertices"].astype(np.float64), m["faces"]
    assert v.shape[1] == 3 and f.shape[1] == 3 and f.min() == 0 and f.max() == len(v) - 1
    assert np.allclose(v.max(0) - v.min(0), [1.2, 0.3, 1.56], atol=0.12)         # the extents of SURVEY App. B
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert area.min() > 0 and 1.0 < area.sum() < 2.0
    assert synth.human_mesh()[2] == "human_obj" and np.array_equal(synth.human_mesh()[0], m["vertices"])
    pts = synth.human_points(200_000, seed=0)
    assert pts.dtype == np.float32 and np.array_equal(pts, synth.human_points(200_000, seed=0))
    assert not np.array_equal(pts[:1000], synth.human_points(1000, seed=1))
    assert np.all(pts.min(0) >= v.min(0) - 1e-6) and np.all(pts.max(0) <= v.max(0) + 1e-6)
    # area-uniform: the share of points above / below a height matches the area share of the triangles there
    zc = (a[:, 2] + b[:, 2] + c[:, 2]) / 3
    for z0 in (-0.4, 0.0, 0.4):
        tri_share = area[zc > z0].sum() / area.sum()
        assert abs((pts[:, 2] > z0).mean() - tri_share) < 0.01
    # every point lies on the surface: distance to its nearest triangle plane ~ 0 (checked on a subsample against ALL triangles)
    sub = pts[:200].astype(np.float64)
    n = np.cross(b - a, c - a); n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = np.abs(((sub[:, None, :] - a[None]) * n[None]).sum(-1))
    assert d.min(1).max() < 1e-6
    cl = synth.init_cloud(1000, 0, "mid", seed=0)                       # "auto" resolves to the asset here
    assert synth.resolve_cloud_source("auto") == "human_obj"
    assert np.array_equal(cl.means3D.numpy(), synth.human_points(1000, 0))
    assert not np.array_equal(synth.init_cloud(1000, 0, "mid", seed=0, source="capsule").means3D.numpy(), cl.means3D.numpy())


def test_cloud_and_mesh_fall_back_to_the_capsule_without_the_local_assets(monkeypatch):
    """the third-party assets are not shipped; without them `init_cloud("auto")`, `human_mesh()` and the motion
    driver use the procedural stand-ins (same extents, same joints, same period) and say so; an explicit request for
    the asset fails loudly."""
    from humangaussian_amd import animation as an, data
    monkeypatch.setattr(data, "HUMAN_MESH", "/nonexistent/human_mesh.npz")
    monkeypatch.setattr(data, "MOTION", "/nonexistent/poses.npz")
    assert synth.resolve_cloud_source("auto") == "capsule"
    cl = synth.init_cloud(2000, 0, "mid", seed=0)
    assert np.array_equal(cl.means3D.numpy(), synth.humanoid_points(2000, 0))
    with pytest.raises(FileNotFoundError):
        synth.init_cloud(100, 0, "mid", source="human_obj")
    v, f, label = synth.human_mesh()
    assert label == "capsule" and v.dtype == np.float32 and f.dtype == np.int32 and f.min() == 0 and f.max() == len(v) - 1
    ext = v.max(0) - v.min(0)
    assert np.allclose(ext, [1.2, 0.3, 1.56], atol=0.12)                # the extents of SURVEY App. B
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert area.min() > 0 and 1.0 < area.sum() < 2.0                    # no degenerate triangle; area like the body's 1.51
    d = an.MotionDriver(v, device="cpu")
    assert d.poses is None and d.num_poses == 136 and "procedural" in d.source
    assert torch.equal(d.vertices(3 + 136), d.vertices(3)) and not torch.equal(d.vertices(3), d.vertices(40))
    verts, anchors = an.human_mesh_anchors(300, seed=1, device="cpu")
    assert verts.shape == v.shape and int(anchors.mapping_face.max()) < len(f)
    with pytest.raises(FileNotFoundError):
        an.MotionDriver(v, device="cpu", poses_path="/nonexistent/clip.npz")


def test_motion_driver_is_driven_by_the_pose_asset_and_anchors_follow_the_mesh(stand_in_assets):
    """configs[4] host pieces: the local pose asset (the reference's content/amass_test_17.npz, 136 x 55 x 3; a stand-in
    clip in the same format here) drives the toy articulation, which is the identity at gain 0, moves limbs but leaves
    the torso (no joint there) in place, and the anchor mapping reproduces animation.py:384-403's formula:
    points = barycentre + dist * face normal."""
    from humangaussian_amd import animation as an
    data = stand_in_assets
    poses = np.load(data.MOTION)["poses"]
    assert poses.shape == (136, 55, 3) and poses.dtype == np.float32 and float(np.abs(poses).max()) < 2 * np.pi
    mesh = np.load(data.HUMAN_MESH)
    d = an.MotionDriver(mesh["vertices"], device="cpu")
    assert d.poses is not None and d.num_poses == 136 and "local asset" in d.source
    assert np.array_equal(d._angles(141), poses[5].astype(np.float64))
    rest = d.rest
    assert torch.equal(an.MotionDriver(mesh["vertices"], device="cpu", gain=0.0).vertices(17), rest)
    v5, v60 = d.vertices(5), d.vertices(60)
    assert torch.equal(d.vertices(5 + 136), v5)                                     # pose i mod 136
    moved = (v60 - v5).norm(dim=1)
    torso = (rest[:, 0].abs() < 0.12) & (rest[:, 2] > 0.05) & (rest[:, 2] < 0.5)
    hands = rest[:, 0].abs() > 0.5
    assert float(moved[torso].max()) < 1e-6 < 0.02 < float(moved[hands].mean())
    assert float((v60 - rest).norm(dim=1).max()) < 0.8                               # stays a body, not an explosion
    verts, anchors = an.human_mesh_anchors(500, seed=4, device="cpu", max_dist=0.004)
    f = anchors.faces.numpy()[anchors.mapping_face.numpy()]
    v0, v1, v2 = (verts[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(v1 - v0, v2 - v0)
    n /= np.linalg.norm(n, axis=1, keepdims=True) + 1e-20
    uvw = anchors.mapping_uvw.numpy().astype(np.float64)
    assert np.allclose(uvw.sum(1), 1.0, atol=1e-6) and uvw.min() >= 0
    pts = v0 * uvw[:, [0]] + v1 * uvw[:, [1]] + v2 * uvw[:, [2]] + anchors.mapping_dist.numpy()[:, None] * n
    assert np.abs(pts).max(0)[2] < 0.79 and float(np.abs(anchors.mapping_dist.numpy()).max()) <= 0.004
