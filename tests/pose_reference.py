"""numpy restatement of the pose-control images (include/hgs_rast.h: hgs_pose_draw; csrc/pose.hip), in two parts:

(a) projection, occlusion and record building - `records_of(..., dtype=np.float64)` is the reference's arithmetic
    (threestudio/utils/poser.py:365-389, :420-445) in float64, `dtype=np.float32` the restatement in the order the header
    states (the fma is emulated through float64: a product of two fp32 values is exact there, the sum is rounded to 53
    bits and then to 24 - a double rounding that can differ from a true fma in the last bit once in ~2^29 cases, which
    is irrelevant for what the restatement is used for, the size of fp32's own error);
(b) `rasterise(records, H, W)`: the integer rules of the header applied to the records, every pixel, no culling.
`capsule_margin` / `ellipse_margin` evaluate the same shapes in float64 for the CPU tests.

The tables come from humangaussian_amd/pose_image.py.  The test skeleton is made up here (rough human proportions plus
noise): the reference's numeric poses are not copied."""
import math

import numpy as np

from humangaussian_amd import pose_image as pi
from humangaussian_amd import synth

EPS32 = float(np.finfo(np.float32).eps)
ONE = 16384
TRIG = [int(np.rint(ONE * math.cos(math.radians(k)))) for k in range(360)]
for _k, _v in ((0, ONE), (90, 0), (180, -ONE), (270, 0)):
    TRIG[_k] = _v
COORD_MAX = 8191.0
CAPSULE, DISC, ELLIPSE = 1, 2, 3
NUM_RECORDS = {"humansd": 16, "openpose": 35}
NUM_KEYPOINTS = {"humansd": 17, "openpose": 18}


def tables(style):
    if style == "humansd":
        return pi.HUMANSD_LIMBS, pi.HUMANSD_COLOURS
    return pi.OPENPOSE_LIMBS, pi.OPENPOSE_COLOURS


def rgb(c):
    return int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16)


# ------------------------------------------------------------------------------------------------- (a) projection

def _fma32(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def project(points, mvp, H, W, dtype=np.float64):
    """points (K, 4), mvp (4, 4) -> xs (K,), ys (K,), z (K,) in `dtype`"""
    with np.errstate(all="ignore"):
        if dtype == np.float64:
            p = np.asarray(points, np.float64) @ np.asarray(mvp, np.float64).T
            ndc = p[:, :3] / p[:, 3:]
            return (ndc[:, 0] + 1) / 2 * H, (ndc[:, 1] + 1) / 2 * W, ndc[:, 2]
        p, m = np.asarray(points, np.float32), np.asarray(mvp, np.float32)
        clip = np.zeros((p.shape[0], 4), np.float32)
        for c in range(4):
            acc = m[c, 0] * p[:, 0]
            for k in (1, 2, 3):
                acc = _fma32(m[c, k], p[:, k], acc)
            clip[:, c] = acc
        ndc = clip[:, :3] / clip[:, 3:]
        one, half = np.float32(1), np.float32(0.5)
        return (ndc[:, 0] + one) * half * np.float32(H), (ndc[:, 1] + one) * half * np.float32(W), ndc[:, 2]


def hidden_keypoints(style, xs, z):
    """the occlusion rules: the set of hidden keypoint indices"""
    el, er, yl, yr = (3, 4, 1, 2) if style == "humansd" else (17, 16, 15, 14)
    if z[0] > z[el] and z[0] < z[er]:
        return {er} | ({yr} if xs[yr] > xs[yl] else set()), "left"
    if z[0] < z[el] and z[0] > z[er]:
        return {el} | ({yl} if xs[yl] < xs[yr] else set()), "right"
    if z[0] > z[el] and z[0] > z[er]:
        return {0, yl, yr}, "back"
    return set(), "none"


def records_of(style, points, mvp, H, W, occlusion=False, limb_width=None, dtype=np.float64):
    """one view -> (records (R, 8) int64, kp (K, 3) in dtype, branch of the occlusion rules)"""
    K, R = NUM_KEYPOINTS[style], NUM_RECORDS[style]
    limbs, colours = tables(style)
    xs, ys, z = project(points, mvp, H, W, dtype)
    hidden, branch = hidden_keypoints(style, xs, z) if occlusion else (set(), "off")
    with np.errstate(all="ignore"):
        usable = (np.abs(xs) <= COORD_MAX) & (np.abs(ys) <= COORD_MAX)
        conf = np.array([0.0 if k in hidden else 1.0 for k in range(K)], dtype)
        if style == "openpose":
            conf = conf * ((xs >= 0) & (xs < H) & (ys >= 0) & (ys < W))
        total = dtype(0)
        for k in range(K):
            total = total + ((xs[k] + ys[k]) + conf[k])
    rec = np.zeros((R, 8), np.int64)
    if style == "humansd":
        w = pi.default_limb_width(H) if limb_width is None else limb_width
        for i, (ci, a, b) in enumerate(limbs):
            if conf[a] > 0.3 and conf[b] > 0.3 and usable[a] and usable[b] and total > 0:
                rec[i] = [CAPSULE, int(xs[a]), int(ys[a]), int(xs[b]), int(ys[b]), w, 0, rgb(colours[ci])]
    else:
        for i in range(K):
            if conf[i] > 0.5:
                rec[i] = [DISC, int(xs[i]), int(ys[i]), 16, 0, 0, 0, rgb(colours[i])]
        half = dtype(0.5)
        for i, (ci, k0, k1) in enumerate(limbs):
            if conf[k0] > 0.5 and conf[k1] > 0.5:
                dx, dy = xs[k0] - xs[k1], ys[k0] - ys[k1]
                length = np.sqrt(dy * dy + dx * dx)
                if dtype == np.float64:
                    angle = math.degrees(math.atan2(dy, dx))
                else:
                    angle = np.arctan2(dy, dx) * np.float32(180.0 / math.pi)
                rec[18 + i] = [ELLIPSE, int((xs[k0] + xs[k1]) * half), int((ys[k0] + ys[k1]) * half), int(length * half),
                               int(angle), 4, 0, rgb(colours[ci])]
    return rec, np.stack([xs, ys, conf], 1).astype(dtype), branch


def fragile_values(style, points, mvp, H, W):
    """the float64 values whose truncation the records depend on: every keypoint coordinate, and for OpenPose every
    limb's centre, length / 2 and angle in degrees (whether or not the limb ends up drawn)"""
    xs, ys, _ = project(points, mvp, H, W)
    vals = list(xs) + list(ys)
    if style == "openpose":
        for _, k0, k1 in pi.OPENPOSE_LIMBS:
            dx, dy = xs[k0] - xs[k1], ys[k0] - ys[k1]
            vals += [(xs[k0] + xs[k1]) / 2, (ys[k0] + ys[k1]) / 2, math.sqrt(dy * dy + dx * dx) / 2,
                     math.degrees(math.atan2(dy, dx))]
    return np.array(vals)


# ----------------------------------------------------------------------------------------------- (b) the rasteriser

def _crop(rec, H, W):
    """a window that holds the record with room to spare - TWICE the reach the rules allow plus 8 pixels - so that the
    rasteriser need not visit every pixel of a 512 x 512 image per record (tests/test_pose_image_cpu.py: same pixels as
    without the window)"""
    t = int(rec[0])
    if t == CAPSULE:
        reach = int(rec[5]) + 8                                  # the rules: 2 d <= w
        xs_, ys_ = (int(rec[1]), int(rec[3])), (int(rec[2]), int(rec[4]))
    else:
        reach = 16 if t == DISC else 2 * max(int(rec[3]), int(rec[5])) + 8
        xs_, ys_ = (int(rec[1]),) * 2, (int(rec[2]),) * 2
    x0, x1 = max(0, min(xs_) - reach), min(W, max(xs_) + reach + 1)
    y0, y1 = max(0, min(ys_) - reach), min(H, max(ys_) + reach + 1)
    return x0, max(x0, x1), y0, max(y0, y1)


def covered(rec, H, W, crop=True):
    """(H, W) bool: the pixels inside one record, by the header's integer rules (numpy int64 throughout)"""
    out = np.zeros((H, W), bool)
    x0, x1, y0, y1 = _crop(rec, H, W) if crop and int(rec[0]) != 0 else (0, W, 0, H)
    if x1 > x0 and y1 > y0:
        out[y0:y1, x0:x1] = _covered(rec, y0, y1, x0, x1)
    return out


def _covered(rec, y0, y1, x0, x1):
    py, px = np.mgrid[y0:y1, x0:x1].astype(np.int64)
    t = int(rec[0])
    if t == CAPSULE:
        ax, ay, bx, by, w = (int(v) for v in rec[1:6])
        apx, apy, abx, aby = px - ax, py - ay, bx - ax, by - ay
        dot, L = apx * abx + apy * aby, abx * abx + aby * aby
        near_a = 4 * (apx * apx + apy * apy) <= w * w
        near_b = 4 * ((px - bx) ** 2 + (py - by) ** 2) <= w * w
        cross = apx * aby - apy * abx
        side = 4 * cross * cross <= w * w * L
        return np.where(dot <= 0, near_a, np.where(dot >= L, near_b, side))
    dx, dy = px - int(rec[1]), py - int(rec[2])
    if t == DISC:
        return dx * dx + dy * dy <= int(rec[3])
    if t == ELLIPSE:
        a, theta, b = int(rec[3]), int(rec[4]), int(rec[5])
        C, S = TRIG[theta % 360], TRIG[(theta - 90) % 360]
        u, v = dx * C + dy * S, dy * C - dx * S
        box = (np.abs(u) <= a * ONE) & (np.abs(v) <= b * ONE)
        u, v = np.where(box, u, 0), np.where(box, v, 0)          # (outside the box the third test is not evaluated)
        return box & (u * u * (b * b) + v * v * (a * a) <= a * a * b * b * ONE * ONE)
    return np.zeros(px.shape, bool)


def rasterise(records, H, W):
    """records (R, 8) of one view -> (H, W, 3) uint8"""
    img = np.zeros((H, W, 3), np.int64)
    for rec in np.asarray(records, np.int64):
        if rec[0] == 0:
            continue
        inside = covered(rec, H, W)
        k = np.array([rec[7] & 255, (rec[7] >> 8) & 255, (rec[7] >> 16) & 255], np.int64)
        if rec[0] == ELLIPSE:
            img[inside] = (4 * img[inside] + 6 * k + 5) // 10
        else:
            img[inside] = k
    return img.astype(np.uint8)


def rasterise_batch(records, H, W):
    return np.stack([rasterise(r, H, W) for r in np.asarray(records)]) if len(records) else np.zeros((0, H, W, 3), np.uint8)


def to_float(img_u8):
    """float32(v) / float32(255), correctly rounded"""
    return img_u8.astype(np.float32) / np.float32(255)


def draw(style, points, mvp, H, W, occlusion=None, limb_width=None, dtype=np.float64):
    """B views -> (images (B, H, W, 3) uint8, kp (B, K, 3), records (B, R, 8)) through (a) in `dtype` and (b)"""
    B = len(mvp)
    occ = [False] * B if occlusion is None else list(occlusion)
    out = [records_of(style, points, mvp[b], H, W, bool(occ[b]), limb_width, dtype) for b in range(B)]
    recs = np.stack([o[0] for o in out])
    return rasterise_batch(recs, H, W), np.stack([o[1] for o in out]), recs


# ------------------------------------------------------------------------- float64 evaluations of the same shapes

def capsule_margin(rec, H, W):
    """4 d^2(P, AB) - w^2 in float64 (<= 0: covered)"""
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    ax, ay, bx, by, w = (float(v) for v in rec[1:6])
    abx, aby = bx - ax, by - ay
    L = abx * abx + aby * aby
    t = np.zeros_like(px) if L == 0 else np.clip(((px - ax) * abx + (py - ay) * aby) / L, 0.0, 1.0)
    qx, qy = ax + t * abx, ay + t * aby
    return 4 * ((px - qx) ** 2 + (py - qy) ** 2) - w * w


def ellipse_margin(rec, H, W):
    """the ellipse with half axes (a, b), turned by the table's fixed-point cosine and sine, in float64: (u / a)^2 +
    (v / b)^2 - 1 for a > 0 (<= 0: covered); for a = 0 the segment u = 0, |v| <= b: returns (margin, exact) where exact
    marks the pixels with u == 0, the only ones the degenerate shape holds"""
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    a, theta, b = int(rec[3]), int(rec[4]), int(rec[5])
    C, S = TRIG[theta % 360] / ONE, TRIG[(theta - 90) % 360] / ONE
    dx, dy = px - float(rec[1]), py - float(rec[2])
    u, v = dx * C + dy * S, dy * C - dx * S
    if a == 0:
        return np.where(u == 0, np.abs(v) - b, 1.0), True
    return (u / a) ** 2 + (v / b) ** 2 - 1.0, False


# ------------------------------------------------------------------------------------------ test skeletons, cameras

_PROPORTIONS = {   # (x = the body's left, depth, height) of a standing figure about 0.55 tall: made up, not the reference's pose
    "nose": (0.0, 0.055, 0.21), "neck": (0.0, 0.0, 0.15), "left_eye": (0.018, 0.045, 0.225), "right_eye": (-0.018, 0.045, 0.225),
    "left_ear": (0.04, 0.0, 0.215), "right_ear": (-0.04, 0.0, 0.215), "left_shoulder": (0.075, 0.0, 0.14),
    "right_shoulder": (-0.075, 0.0, 0.14), "left_elbow": (0.12, -0.01, 0.06), "right_elbow": (-0.12, -0.01, 0.06),
    "left_wrist": (0.16, 0.03, -0.02), "right_wrist": (-0.16, 0.03, -0.02), "left_hip": (0.045, 0.0, -0.03),
    "right_hip": (-0.045, 0.0, -0.03), "left_knee": (0.05, 0.01, -0.16), "right_knee": (-0.05, 0.01, -0.16),
    "left_ankle": (0.052, 0.0, -0.29), "right_ankle": (-0.052, 0.0, -0.29)}


def make_skeleton(style, seed=0, noise=0.004):
    """(K, 4) fp32 homogeneous keypoints, z up (the reference's swapped axes)"""
    names = pi.HUMANSD_NAMES if style == "humansd" else pi.OPENPOSE_NAMES
    rng = np.random.default_rng(seed)
    p = np.array([_PROPORTIONS[n] for n in names]) + rng.normal(size=(len(names), 3)) * noise
    return np.concatenate([p, np.ones((len(names), 1))], 1).astype(np.float32)


def orbit_mvp(elev, azim, dist, fovy, H, W):
    """the reference's mvp convention (points @ mvp.T) of an orbit camera of humangaussian_amd.synth, as fp32"""
    return synth.orbit_camera(elev, azim, dist, fovy, H, W).full_proj_transform.numpy().T.copy()


SAMPLER_MARGIN = 0.02
SAMPLER_TRIES = 5000


def sample_views(style, H, W, B, seed, points=None):
    """B orbit cameras (fixed seed, the ranges of synth.random_cameras) drawn by rejection until every value of
    `fragile_values` is at least SAMPLER_MARGIN from an integer in float64 - then fp32 cannot truncate differently.
    points: the skeleton (K, 4) the condition is about (default: make_skeleton(style, seed)).
    Returns (points (K, 4), mvp (B, 4, 4) fp32, tries); raises if SAMPLER_TRIES draws do not fill the quota."""
    rng = np.random.default_rng(seed)
    points = make_skeleton(style, seed) if points is None else np.asarray(points, np.float32)
    out, tries = [], 0
    while len(out) < B:
        tries += 1
        if tries > SAMPLER_TRIES:
            raise RuntimeError(f"sample_views: {len(out)} of {B} views after {SAMPLER_TRIES} draws")
        m = orbit_mvp(rng.uniform(-30, 30), rng.uniform(-180, 180), rng.uniform(1.5, 2.0), rng.uniform(40, 70), H, W)
        vals = fragile_values(style, points, m, H, W)
        if np.all(np.abs(vals - np.rint(vals)) >= SAMPLER_MARGIN):
            out.append(m)
    return points, np.stack(out).astype(np.float32), tries
