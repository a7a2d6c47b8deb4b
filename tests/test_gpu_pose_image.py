"""GPU tests of the pose-control images (csrc/pose.hip, humangaussian_amd/pose_image.py).

What the kernel is held to (tests/pose_reference.py):
  raster    the image equals the integer rasteriser applied to the kernel's OWN records, every pixel, both dtypes;
  records   equal the float64 records exactly, on views drawn so that no truncated value is within 0.02 of an integer;
  kp        max |error| of xs, ys against float64 <= 4 x the fp32 restatement's own error, floor 16 eps32 max(H, W) (the
            factor 4: fma contraction and the division, not a measured bound).  HGS_WRITE_PROFILES=1 records the ratios in
            profiles/pose_image_parity.json.
Shapes: (64, 64) whole tiles, (52, 75) partial tiles both ways, W % 4 != 0 and rows that are not 16-byte aligned, (97, 130)
non-square with several tile rows, (512, 512) the size of a training step."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import lbs_reference as lr
import pose_reference as pr
from humangaussian_amd import _lib, body
from humangaussian_amd import pose_image as pi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SHAPES = [(64, 64), (52, 75), (97, 130), (512, 512)]
STYLES = ["openpose", "humansd"]
# the views of the records test (tests/test_pose_image_cpu.py asserts that the sampler fills these quotas)
RECORD_CASES = [("openpose", 64, 64, 3, 11), ("openpose", 97, 130, 8, 12), ("openpose", 512, 512, 8, 13),
                ("humansd", 64, 64, 3, 21), ("humansd", 97, 130, 8, 22), ("humansd", 512, 512, 8, 23)]

_VIEWS, _RASTER = {}, {}


def _views(style, H, W, B=8):
    """the skeleton and B sampled cameras of a (style, shape), built once"""
    key = (style, H, W, B)
    if key not in _VIEWS:
        seed = 100 + 10 * SHAPES.index((H, W)) + STYLES.index(style) if (H, W) in SHAPES else 7
        _VIEWS[key] = pr.sample_views(style, H, W, B, seed)[:2]
    return _VIEWS[key]


def _raster(records, H, W):
    """rasteriser (b) on one view's records, cached by the records' bytes"""
    rec = np.ascontiguousarray(records, np.int64)
    key = (H, W, rec.tobytes())
    if key not in _RASTER:
        _RASTER[key] = pr.rasterise(rec, H, W)
    return _RASTER[key]


def _expect(records, H, W):
    return np.stack([_raster(r, H, W) for r in records.cpu().numpy()])


def _check_image(image, records, H, W):
    want = _expect(records, H, W)
    if image.dtype == torch.uint8:
        assert torch.equal(image.cpu(), torch.from_numpy(want))
    else:
        assert torch.equal(image.cpu(), torch.from_numpy(pr.to_float(want)))


def _skeleton(style, points):
    return pi.PoseSkeleton(points, humansd_style=style == "humansd", device=DEV)


# ------------------------------------------------------------------------------------------------ 1. raster exactness

@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("style", STYLES)
def test_image_equals_the_integer_rasteriser_on_the_kernels_own_records(style, shape):
    H, W = shape
    points, mvp = _views(style, H, W)
    sk = _skeleton(style, points)
    m = torch.from_numpy(mvp).to(DEV)
    drawn = 0
    for B in (1, 3, 8):
        for width in (1, 2, 7, None):
            for dtype in (torch.float32, torch.uint8):
                occ = torch.arange(B, device=DEV) % 2 == 1
                image, kp, records = sk.draw_views(m[:B], H, W, enable_occlusion=occ, limb_width=width, dtype=dtype,
                                                   return_records=True)
                assert image.shape == (B, H, W, 3) and image.dtype == dtype and image.device.type == DEV
                assert kp.shape == (B, len(points), 3) and records.shape == (B, pr.NUM_RECORDS[style], 8)
                _check_image(image, records, H, W)
                drawn += int((image != 0).sum())
                if style == "humansd":
                    w = pi.default_limb_width(H) if width is None else width
                    live = records[:, :, 0] != 0
                    assert bool((records[:, :, 5][live] == w).all()) and bool(live.any())
    assert drawn > 0


# ------------------------------------------------------------------------------------------------------ 2. records

@pytest.mark.parametrize("case", RECORD_CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}_B{c[3]}" for c in RECORD_CASES])
def test_records_equal_the_float64_records(case):
    style, H, W, B, seed = case
    points, mvp, _ = pr.sample_views(style, H, W, B, seed)
    occ = [b % 2 == 0 for b in range(B)]
    _, kp, records = _skeleton(style, points).draw_views(torch.from_numpy(mvp).to(DEV), H, W, enable_occlusion=np.array(occ),
                                                         limb_width=3, return_records=True)
    want_img, want_kp, want = pr.draw(style, points, mvp, H, W, occlusion=occ, limb_width=3)
    assert np.array_equal(records.cpu().numpy().astype(np.int64), want)
    assert np.array_equal(kp[:, :, 2].cpu().numpy().astype(np.float64), want_kp[:, :, 2])          # conf / mask
    assert (want[:, :, 0] != 0).sum() >= 0.8 * want.shape[0] * want.shape[1]


# ------------------------------------------------------------------------------------------------- 3. kp against fp64

_RATIOS = {}


def _record_ratios(case_id, entry):
    _RATIOS[case_id] = entry
    if not os.environ.get("HGS_WRITE_PROFILES"):
        return
    doc = {"what": "per case of tests/test_gpu_pose_image.py: max |error| of hgs_pose_draw's xs, ys against the float64 "
                   "projection, the fp32 restatement's own error, both in units of eps32 max(H, W), and the gate "
                   "max(4 ref, 16) the first is held to",
           "device": torch.cuda.get_device_name(0), "cases": dict(sorted(_RATIOS.items()))}
    with open(os.path.join(ROOT, "profiles", "pose_image_parity.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("style", STYLES)
def test_kp_against_fp64(style, shape):
    H, W = shape
    points, mvp = _views(style, H, W)
    _, kp = _skeleton(style, points).draw_views(torch.from_numpy(mvp).to(DEV), H, W, limb_width=1)
    got = kp.cpu().numpy().astype(np.float64)
    err = ref = 0.0
    for b in range(len(mvp)):
        x64, y64, _ = pr.project(points, mvp[b], H, W)
        x32, y32, _ = pr.project(points, mvp[b], H, W, np.float32)
        err = max(err, np.abs(got[b, :, 0] - x64).max(), np.abs(got[b, :, 1] - y64).max())
        ref = max(ref, np.abs(x32 - x64).max(), np.abs(y32 - y64).max())
    unit = pr.EPS32 * max(H, W)
    gate = max(4.0 * ref, 16.0 * unit)
    entry = {"hip_over_unit": err / unit, "ref_over_unit": ref / unit, "gate_over_unit": gate / unit,
             "hip_over_ref": err / ref if ref > 0 else (0.0 if err == 0 else float("inf"))}
    print(style, shape, entry)
    _record_ratios(f"{style}_{H}x{W}", entry)
    assert err <= gate, entry


# --------------------------------------------------------------------------------------------- 4. hand-built edge cases

EYE = np.eye(4, dtype=np.float32)


def _points_at(xy, H, W, z=None, w=None):
    """keypoints that the identity mvp puts at (xs, ys) = xy: x = 2 xs / H - 1, y = 2 ys / W - 1 (x goes with H, as the
    reference has it).  Targets at pixel centres (n + 0.5) truncate safely."""
    xy = np.asarray(xy, np.float64)
    p = np.ones((len(xy), 4))
    p[:, 0], p[:, 1] = 2 * xy[:, 0] / H - 1, 2 * xy[:, 1] / W - 1
    p[:, 2] = 0.0 if z is None else z
    if w is not None:
        p[:, 3] = w
    return p.astype(np.float32)


def _draw_and_check(style, points, mvp, H, W, occlusion=False, limb_width=None, compare_records=None):
    """both dtypes against rasteriser (b) on the kernel's records; the records against the float64 ones where the inputs
    allow it: by default for HumanSD, whose hand-built keypoints sit at pixel centres (an OpenPose limb's centre, half
    length and angle between such points can be whole numbers, which fp32 may truncate the other way)"""
    if compare_records is None:
        compare_records = style == "humansd"
    sk = _skeleton(style, points)
    m = torch.from_numpy(np.asarray(mvp, np.float32).reshape(-1, 4, 4)).to(DEV)
    out = {}
    for dtype in (torch.float32, torch.uint8):
        image, kp, records = sk.draw_views(m, H, W, enable_occlusion=occlusion, limb_width=limb_width, dtype=dtype,
                                           return_records=True)
        _check_image(image, records, H, W)
        out[dtype] = image
    torch.cuda.synchronize()
    rec = records.cpu().numpy().astype(np.int64)
    if compare_records:
        occ = [bool(occlusion)] * len(m) if isinstance(occlusion, (bool, np.bool_)) else list(occlusion)
        want = pr.draw(style, points, m.cpu().numpy(), H, W, occlusion=occ, limb_width=limb_width)[2]
        assert np.array_equal(rec, want)
    return out[torch.uint8].cpu().numpy(), rec, kp.cpu().numpy()


def _grid_skeleton(style, H, W):
    """every keypoint at its own pixel centre inside the image"""
    K = pr.NUM_KEYPOINTS[style]
    rng = np.random.default_rng(5)
    return np.stack([rng.integers(8, H - 8, K) + 0.5, rng.integers(8, W - 8, K) + 0.5], 1)


@pytest.mark.parametrize("style", STYLES)
def test_limb_of_length_zero(style):
    H = W = 96
    xy = _grid_skeleton(style, H, W)
    a, b = (5, 7) if style == "humansd" else (2, 3)          # left shoulder - left elbow / right shoulder - right elbow
    xy[b] = xy[a]
    img, rec, _ = _draw_and_check(style, _points_at(xy, H, W), EYE, H, W, limb_width=7)
    if style == "humansd":
        i = pi.HUMANSD_LINES.index((a, b))
        assert rec[0, i, 0] == pr.CAPSULE and tuple(rec[0, i, 1:3]) == tuple(rec[0, i, 3:5])
    else:
        i = 18 + pi.OPENPOSE_LINES.index((a, b))
        assert rec[0, i, 0] == pr.ELLIPSE and rec[0, i, 3] == 0 and rec[0, i, 4] == 0      # a = 0, atan2(0, 0) = 0
    assert img.any()


def test_crossing_limbs_take_the_later_colour():
    """the last two limbs of the table cross: nothing is drawn after them"""
    H = W = 96
    xy = np.tile([[90.5, 90.5]], (17, 1))                    # everything else: zero-length limbs in a corner
    xy[13], xy[15] = (20.5, 30.5), (70.5, 30.5)              # limb 14: left knee - left ankle, horizontal
    xy[14], xy[16] = (45.5, 10.5), (45.5, 60.5)              # limb 15: right knee - right ankle, vertical, drawn later
    assert pi.HUMANSD_LINES[14] == (13, 15) and pi.HUMANSD_LINES[15] == (14, 16)
    img, rec, _ = _draw_and_check("humansd", _points_at(xy, H, W), EYE, H, W, limb_width=5)
    c14, c15 = pi.HUMANSD_COLOURS[pi.HUMANSD_LIMBS[14][0]], pi.HUMANSD_COLOURS[pi.HUMANSD_LIMBS[15][0]]
    assert tuple(img[0, 30, 45]) == c15 and tuple(img[0, 30, 25]) == c14 and tuple(img[0, 15, 45]) == c15
    assert tuple(img[0, 32, 45]) == c15 and tuple(img[0, 32, 48]) == c14 and tuple(img[0, 33, 50]) == (0, 0, 0)


def test_five_limbs_blend_at_the_neck():
    H, W = 97, 130
    points, mvp = _views("openpose", H, W)
    img, rec, _ = _draw_and_check("openpose", points, mvp[:1], H, W, compare_records=True)       # (sampled views: safe)
    at_neck = [18 + i for i, (a, b) in enumerate(pi.OPENPOSE_LINES) if 1 in (a, b)]
    assert len(at_neck) == 5 and (rec[0, at_neck, 0] == pr.ELLIPSE).all()
    # pixels that more than one limb covers exist, and their colour is no limb's own 0.6 k
    cover = sum(pr.covered(rec[0, i], H, W).astype(int) for i in at_neck)
    assert cover.max() >= 2


def test_humansd_keypoints_outside_the_image_far_away_and_behind():
    H = W = 96
    xy = _grid_skeleton("humansd", H, W)
    xy[9], xy[10] = (-25.5, 40.5), (W + 25.5, 50.5)          # wrists: left and right of the image
    xy[15], xy[16] = (30.5, -30.5), (60.5, H + 30.5)         # ankles: above and below
    xy[3] = (9000.5, 20.5)                                   # left ear beyond 8191
    w = np.ones(17)
    points = _points_at(xy, H, W, w=w)
    points[4] = (0.5, 0.25, 0.0, 0.0)                        # right ear: w = 0, xs = ys = +inf
    points[0] = (-0.3, -0.2, 0.0, -1e-5)                     # nose: w < 0, lands far away (positive side)
    img, rec, kp = _draw_and_check("humansd", points, EYE, H, W, limb_width=4)
    assert np.isinf(kp[0, 4, 0]) and np.isinf(kp[0, 4, 1]) and kp[0, 0, 0] > 8191 and kp[0, 3, 0] > 8191
    for i, (a, b) in enumerate(pi.HUMANSD_LINES):
        dead = bool({a, b} & {0, 3, 4})
        assert (rec[0, i, 0] == 0) == dead and (not dead or not rec[0, i].any()), (i, a, b)
    assert sum(1 for a, b in pi.HUMANSD_LINES if {a, b} & {0, 3, 4}) == 6
    # the limbs that leave the image are drawn up to its edge
    assert img[0, :, 0].any() and img[0, :, W - 1].any() and img[0, 0].any() and img[0, H - 1].any()


@pytest.mark.parametrize("style", STYLES)
def test_view_with_every_limb_invalid_is_all_zeros(style):
    H = W = 64
    xy = np.tile([[-200.5, -300.5]], (pr.NUM_KEYPOINTS[style], 1))        # usable, but the view's sum is negative
    good = _grid_skeleton(style, H, W)
    sk_pts = _points_at(good, H, W)
    shift = EYE.copy()
    shift[0, 3], shift[1, 3] = -2.0 * (good[:, 0].max() + 200) / H, -2.0 * (good[:, 1].max() + 300) / W   # view 1: all off-image
    img, rec, kp = _draw_and_check(style, sk_pts, np.stack([EYE, shift]), H, W, limb_width=3, compare_records=False)
    assert img[0].any() and not img[1].any() and not rec[1].any() and rec[0].any()
    img2, rec2, _ = _draw_and_check(style, _points_at(xy, H, W), EYE, H, W, limb_width=3)
    assert not img2.any() and not rec2.any()
    nan_view = np.zeros((4, 4), np.float32)                                # clip = 0: 0 / 0 everywhere
    img3, rec3, kp3 = _draw_and_check(style, sk_pts, nan_view, H, W, limb_width=3, compare_records=False)
    assert not img3.any() and not rec3.any() and np.isnan(kp3[0, :, :2]).all()


@pytest.mark.parametrize("style", STYLES)
def test_occlusion_branches_with_mixed_flags(style):
    """ndc z = alpha x + beta y by the view's third row: the nose between, in front of or behind the ears at will"""
    H = W = 96
    K = pr.NUM_KEYPOINTS[style]
    names = pi.HUMANSD_NAMES if style == "humansd" else pi.OPENPOSE_NAMES
    xy = _grid_skeleton(style, H, W)
    place = {"nose": (48.5, 30.5), "left_ear": (60.5, 40.5), "right_ear": (36.5, 40.5), "left_eye": (53.5, 26.5), "right_eye": (43.5, 26.5)}
    for n, v in place.items():
        xy[names.index(n)] = v
    points = _points_at(xy, H, W)
    views, want_branch = [], []
    for branch, (alpha, beta) in (("right", (1.0, 0.0)), ("left", (-1.0, 0.0)), ("back", (0.0, -1.0)), ("none", (0.0, 1.0))):
        for flip in (1.0, -1.0):                             # flip mirrors x: both outcomes of the eye comparison
            m = EYE.copy()
            m[0, 0] = flip
            m[2] = (alpha, beta, 0.0, 0.0)
            views.append(m)
            want_branch.append(branch)
    views = np.stack(views)
    for flags in ([True] * 8, [False] * 8, [True, False] * 4, [False, True, True, False, True, False, False, True]):
        img, rec, kp = _draw_and_check(style, points, views, H, W, occlusion=np.array(flags), limb_width=3)
        for b in range(8):
            _, kp64, branch = pr.records_of(style, points, views[b], H, W, occlusion=flags[b], limb_width=3)
            assert branch == (want_branch[b] if flags[b] else "off")
            assert np.array_equal(kp[b, :, 2].astype(np.float64), kp64[:, 2])
    hidden = [K - int(kp[b, :, 2].sum()) for b in range(8)]       # the last call: flags F T T F T F F T
    assert hidden[0] == 0 and hidden[3] == 0 and hidden[7] == 0 and hidden[4] == 3 and {hidden[1], hidden[2]} == {1, 2}


# ----------------------------------------------------------------------------------- 5. no write outside the buffers

@pytest.mark.parametrize("style,uint8_out,shift", [("humansd", 1, 0), ("humansd", 1, 1), ("humansd", 0, 0), ("humansd", 0, 4),
                                                   ("openpose", 0, 0), ("openpose", 1, 3)])
def test_raw_abi_call_leaves_the_guard_rows_intact_and_writes_every_byte(style, uint8_out, shift):
    H, W, B = 52, 75, 3
    lib = _lib.load()
    points, mvp = _views(style, H, W)
    K, R = len(points), pr.NUM_RECORDS[style]
    GUARD = 4096
    sizes = {"image": B * H * W * 3 * (1 if uint8_out else 4), "kp": B * K * 3 * 4, "records": B * R * 8 * 4}
    assert lib.hgs_pose_records_bytes(_lib.POSE_HUMANSD if style == "humansd" else _lib.POSE_OPENPOSE, B) == sizes["records"]
    bufs = {k: torch.full((GUARD + shift + n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV) for k, n in sizes.items()}
    start = {"image": GUARD + shift, "kp": GUARD, "records": GUARD}
    pts, m = torch.from_numpy(points).to(DEV), torch.from_numpy(mvp[:B]).to(DEV).contiguous()
    occ = torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV)
    a = _lib.HgsPoseArgs()
    a.style = _lib.POSE_HUMANSD if style == "humansd" else _lib.POSE_OPENPOSE
    a.B, a.K, a.H, a.W, a.limb_width, a.uint8_out = B, K, H, W, 2, uint8_out
    a.points, a.mvp, a.occlusion = pts.data_ptr(), m.data_ptr(), occ.data_ptr()
    for k in sizes:
        setattr(a, k, bufs[k].data_ptr() + start[k])
    stream = torch.cuda.current_stream()
    rc = lib.hgs_pose_draw(ctypes.byref(a), ctypes.c_void_p(stream.cuda_stream))
    stream.synchronize()
    assert rc == 0
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, n in sizes.items():
        assert (host[k][:start[k]] == 0xFF).all() and (host[k][start[k] + n:] == 0xFF).all(), k
    records = np.frombuffer(host["records"][GUARD:GUARD + sizes["records"]].tobytes(), np.int32).reshape(B, R, 8)
    kp = np.frombuffer(host["kp"][GUARD:GUARD + sizes["kp"]].tobytes(), np.float32)
    assert np.isfinite(kp).all()                                            # 0xFFFFFFFF is a NaN: every float was written
    raw = host["image"][start["image"]:start["image"] + sizes["image"]].tobytes()
    want = np.stack([_raster(r, H, W) for r in records])
    if uint8_out:
        image = np.frombuffer(raw, np.uint8).reshape(B, H, W, 3)
        assert np.array_equal(image, want)
        if style == "humansd":
            assert (image != 0xFF).all() and (records != -1).all()         # no palette channel is 255: every byte was written
    else:
        image = np.frombuffer(raw, np.float32).reshape(B, H, W, 3)
        assert not np.isnan(image).any() and np.array_equal(image, pr.to_float(want))
    assert want.any()


# ------------------------------------------------------------------------------- 6. batch invariance and determinism

@pytest.mark.parametrize("style", STYLES)
def test_view_of_a_batch_is_bit_equal_to_its_own_call_and_calls_repeat(style):
    H, W = 97, 130
    points, mvp = _views(style, H, W)
    sk = _skeleton(style, points)
    m = torch.from_numpy(mvp).to(DEV)
    occ = torch.tensor([1, 0, 0, 1, 1, 0, 1, 0], dtype=torch.bool, device=DEV)
    kw = dict(limb_width=3, return_records=True)
    first = sk.draw_views(m, H, W, enable_occlusion=occ, **kw)
    again = sk.draw_views(m, H, W, enable_occlusion=occ, **kw)
    for x, y in zip(first, again):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for b in range(8):
        one = sk.draw_views(m[b:b + 1], H, W, enable_occlusion=occ[b:b + 1], **kw)
        for x, y in zip(first, one):
            assert torch.equal(x[b].view(torch.int32), y[0].view(torch.int32)), b


# -------------------------------------------------------------------------------------------------------- 7. end to end

@pytest.mark.parametrize("style", STYLES)
def test_body_to_control_images_equals_the_numpy_path_on_the_same_joints(style):
    H = W = 128
    b = lr.make_body(90, 55, "smplx", 4, True, seed=130)
    sb = body.SkinnedBody(b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"], posedirs=b["posedirs"],
                          device=DEV)
    pose = lr.make_poses("random", 1, 55, seed=131)[0] * np.float32(0.2)
    ids = [3, 81, 40, 17, 66]                                # stand-ins for the nose, eye and ear vertices
    humansd = style == "humansd"
    sk, centre, scale = pi.PoseSkeleton.from_body(sb, pose, ids, humansd_style=humansd)
    # the same steps spelled out: pose -> extra_joints -> keypoints_from_joints -> the swap
    v, j = sb.pose(pose, centre=centre, scale=scale, return_joints=True)
    joints = torch.cat([j[0], body.SkinnedBody.extra_joints(v[0], ids)], 0)
    assert joints.shape == (60, 3)
    kps = pi.keypoints_from_joints(joints, style)
    assert torch.equal(sk.points3D[:, :3], kps[:, [0, 2, 1]]) and bool((sk.points3D[:, 3] == 1).all())
    side = (v[0].max(0).values - v[0].min(0).values).max().item()
    assert abs(side - 0.6) < 1e-4
    wrists = [sk.name.index("left_wrist"), sk.name.index("right_wrist")]
    assert torch.equal(sk.hand_centers, sk.points3D[wrists, :3]) and sk.hand_centers.device.type == "cuda"
    # the numpy path on the same joints, cameras drawn for them
    jn = joints.cpu().numpy()
    pts = np.concatenate([pi.keypoints_from_joints(jn, style)[:, [0, 2, 1]], np.ones((len(kps), 1), np.float32)], 1)
    assert np.array_equal(pts, sk.points3D.cpu().numpy())
    _, mvp, _ = pr.sample_views(style, H, W, 3, 140, points=pts)
    image, kp = sk.draw_views(torch.from_numpy(mvp).to(DEV), H, W, enable_occlusion=True, limb_width=3, dtype=torch.uint8)
    want, want_kp, _ = pr.draw(style, pts, mvp, H, W, occlusion=[True] * 3, limb_width=3)
    assert np.array_equal(image.cpu().numpy(), want) and want.any()
    # and the reference's one-view signatures
    if humansd:
        one, kp1 = sk.humansd_draw(mvp[0], H, W, enable_occlusion=True)
        assert kp1.shape == (1, 17, 3) and one.shape == (H, W, 3) and one.dtype == torch.float32
        want1 = pr.draw(style, pts, mvp[:1], H, W, occlusion=[True])[0][0]                 # the default width int(10 H / 512)
        assert torch.equal(one.cpu(), torch.from_numpy(pr.to_float(want1)))
        with pytest.raises(ValueError):
            sk.draw(mvp[0], H, W)
    else:
        one, kp1 = sk.draw(torch.from_numpy(mvp[0]).to(DEV), H, W, enable_occlusion=True)
        assert kp1.shape == (18, 2) and torch.equal(one.cpu(), torch.from_numpy(pr.to_float(want[0])))
        with pytest.raises(ValueError):
            sk.humansd_draw(mvp[0], H, W)


# ----------------------------------------------------------------------------------------------------------- errors

def test_cpu_tensors_bad_shapes_and_widths_raise():
    points = pr.make_skeleton("humansd", 1)
    sk = _skeleton("humansd", points)
    m = torch.eye(4, device=DEV)[None]
    with pytest.raises(RuntimeError, match="HIP device"):
        sk.draw_views(torch.eye(4)[None], 64, 64)
    with pytest.raises(RuntimeError, match="HIP device"):
        sk.draw_views(m, 64, 64, enable_occlusion=torch.ones(1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="HIP device"):
        pi.PoseSkeleton(torch.zeros(17, 3), humansd_style=True, device=DEV)
    with pytest.raises(ValueError, match="limb_width"):
        sk.draw_views(m, 51, 64)                             # int(10 * 51 / 512) = 0
    with pytest.raises(ValueError, match="limb_width"):
        sk.draw_views(m, 64, 64, limb_width=0)
    with pytest.raises(ValueError):
        sk.draw_views(m, 4097, 64)
    with pytest.raises(ValueError):
        sk.draw_views(m, 64, 0)
    with pytest.raises(ValueError):
        sk.draw_views(torch.zeros(2, 3, 4, device=DEV), 64, 64)
    with pytest.raises(ValueError):
        sk.draw_views(m, 64, 64, enable_occlusion=np.array([True, False]))
    with pytest.raises(ValueError):
        pi.PoseSkeleton(points, humansd_style=False, device=DEV)           # 17 points for the 18-point style
    with pytest.raises(RuntimeError):
        _lib.load_binding().pose_draw(sk.points3D, m, None, 0, 64, 64, 1, False)           # K does not fit the style
    with pytest.raises(RuntimeError):
        _lib.load_binding().pose_draw(sk.points3D, m, None, 1, 64, 64, 0, False)
    # an empty batch is an empty result, without a launch
    image, kp = sk.draw_views(torch.zeros(0, 4, 4, device=DEV), 64, 64)
    assert image.shape == (0, 64, 64, 3) and kp.shape == (0, 17, 3)
    torch.cuda.synchronize()
