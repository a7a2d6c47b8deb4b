"""numpy restatement of the rotation-carrying re-anchoring pass (include/hgs_rast.h: hgs_reanchor_rot) and the small meshes
its tests use.

Quaternions are (w, x, y, z).  R(q) is the reference's build_rotation (gaussiansplatting/utils/general_utils.py:78-99) of
q / |q|;  p (x) q the Hamilton product, R(p (x) q) = R(p) R(q).  Frame of a face (a, b, c):

    e1 = (b - a) / |b - a|,   n = (b - a) x (c - a) / |(b - a) x (c - a)|,   e2 = n x e1,   F = [e1 e2 n] (columns)
    r(a, b, c) = a unit quaternion of F, from the largest of the four terms 1 +- F00 +- F11 +- F22
    r = (1, 0, 0, 0)  where |b - a|^2 or |(b - a) x (c - a)|^2 is below 1e-30 or not finite

    bind:  rot_base[i] = conj(r(rest face of i)) (x) rot_raw[i]         pose:  rot[i] = r(posed face of i) (x) rot_base[i]

One implementation, two number formats: `*_fp64` is the yardstick, `*_fp32` rounds every operation to fp32 in the order
the kernel (csrc/bookkeeping.hip: hgs_reanchor_rot_body) performs it - numpy rounds each array operation, sqrt and division
included, to the array's format - so it is the kernel's arithmetic up to the last places of sqrtf and of the division.
Inputs are fp32 arrays in both forms (what the kernel reads); the fp64 form converts them exactly."""
import numpy as np

EPS_FACE = 1e-30
F_MAX = float(np.finfo(np.float32).max)


# ---------------------------------------------------------------------------------------------------- the definitions

def hamilton(p, q):
    pw, px, py, pz = (p[:, k] for k in range(4))
    qw, qx, qy, qz = (q[:, k] for k in range(4))
    return np.stack([((pw * qw - px * qx) - py * qy) - pz * qz,
                     ((pw * qx + px * qw) + py * qz) - pz * qy,
                     ((pw * qy - px * qz) + py * qw) + pz * qx,
                     ((pw * qz + px * qy) - py * qx) + pz * qw], 1)


def conj(q):
    return q * np.array([1, -1, -1, -1], q.dtype)


def face_quat(a, b, c):
    """(N,3) x 3 of one dtype -> (N,4) of that dtype: r(a, b, c), every operation in the kernel's order"""
    dt = a.dtype
    one, half = dt.type(1), dt.type(0.5)
    with np.errstate(all="ignore"):
        d1, d2 = b - a, c - a
        mx = d1[:, 1] * d2[:, 2] - d1[:, 2] * d2[:, 1]
        my = d1[:, 2] * d2[:, 0] - d1[:, 0] * d2[:, 2]
        mz = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
        mm = (mx * mx + my * my) + mz * mz
        ll = (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]) + d1[:, 2] * d1[:, 2]
        lo, hi = dt.type(EPS_FACE), dt.type(F_MAX)
        sound = (ll >= lo) & (ll <= hi) & (mm >= lo) & (mm <= hi)
        l, m = np.sqrt(ll), np.sqrt(mm)
        f00, f10, f20 = d1[:, 0] / l, d1[:, 1] / l, d1[:, 2] / l
        f02, f12, f22 = mx / m, my / m, mz / m
        f01, f11, f21 = f12 * f20 - f22 * f10, f22 * f00 - f02 * f20, f02 * f10 - f12 * f00
        tw, tx = ((one + f00) + f11) + f22, ((one + f00) - f11) - f22
        ty, tz = ((one - f00) + f11) - f22, ((one - f00) - f11) + f22
        pw = (tw >= tx) & (tw >= ty) & (tw >= tz)
        px = ~pw & (tx >= ty) & (tx >= tz)
        py = ~pw & ~px & (ty >= tz)
        t = np.where(pw, tw, np.where(px, tx, np.where(py, ty, tz)))
        s = np.sqrt(t)
        big, h = half * s, half / s
        dw, dy, dz = f21 - f12, f02 - f20, f10 - f01
        sxy, sxz, syz = f01 + f10, f02 + f20, f12 + f21
        rw = np.where(pw, big, np.where(px, dw, np.where(py, dy, dz)) * h)
        rx = np.where(px, big, np.where(pw, dw, np.where(py, sxy, sxz)) * h)
        ry = np.where(py, big, np.where(pw, dy, np.where(px, sxy, syz)) * h)
        rz = np.where(pw | px | py, np.where(pw, dz, np.where(px, sxz, syz)) * h, big)
    r = np.stack([rw, rx, ry, rz], 1)
    r[~sound] = np.array([1, 0, 0, 0], dt)
    return r.astype(dt)


def _corners(vertices, faces, mapping_face, dt):
    v = np.asarray(vertices, np.float32).astype(dt)
    tri = np.asarray(faces)[np.asarray(mapping_face)]
    return v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]


def _bind(vertices, faces, mapping_face, rot_raw, dt):
    return hamilton(conj(face_quat(*_corners(vertices, faces, mapping_face, dt))), np.asarray(rot_raw, np.float32).astype(dt))


def _pose(vertices, faces, mapping_face, rot_base, dt):
    return hamilton(face_quat(*_corners(vertices, faces, mapping_face, dt)), np.asarray(rot_base).astype(dt))


def bind_fp64(vertices, faces, mapping_face, rot_raw):
    return _bind(vertices, faces, mapping_face, rot_raw, np.dtype(np.float64))


def pose_fp64(vertices, faces, mapping_face, rot_base):
    return _pose(vertices, faces, mapping_face, rot_base, np.dtype(np.float64))


def bind_fp32(vertices, faces, mapping_face, rot_raw):
    return _bind(vertices, faces, mapping_face, rot_raw, np.dtype(np.float32))


def pose_fp32(vertices, faces, mapping_face, rot_base):
    return _pose(vertices, faces, mapping_face, rot_base, np.dtype(np.float32))


def repose_fp64(rest, posed, faces, mapping_face, rot_raw):
    """bind at `rest`, pose at `posed`, all in fp64 (the fp64 rot_base is NOT rounded to fp32 in between)"""
    return pose_fp64(posed, faces, mapping_face, bind_fp64(rest, faces, mapping_face, rot_raw))


def repose_fp32(rest, posed, faces, mapping_face, rot_raw):
    return pose_fp32(posed, faces, mapping_face, bind_fp32(rest, faces, mapping_face, rot_raw))


def rotmat(q):
    """(N,4) -> (N,3,3) float64: build_rotation of q / |q|"""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def positions_fp64(vertices, faces, mapping_face, uvw, dist):
    """xyz of hgs_reanchor in fp64 (animation.py:384-403)"""
    a, b, c = _corners(vertices, faces, mapping_face, np.dtype(np.float64))
    n = np.cross(b - a, c - a)
    n = n / (np.linalg.norm(n, axis=1, keepdims=True) + 1e-20)
    uvw = np.asarray(uvw, np.float64)
    return a * uvw[:, :1] + b * uvw[:, 1:2] + c * uvw[:, 2:] + np.asarray(dist, np.float64)[:, None] * n


# ---------------------------------------------------------------------------------------------------- the small meshes

NUM_FACES = 40
SIZES = (1, 255, 256, 257, 1025)          # one thread, and either side of one / four 256-thread workgroups
EDGE_MIN, EDGE_MAX, ANGLE_MIN = 0.01, 0.1, 20.0


def _angles(a, b, c):
    out = []
    for p, q, r in ((a, b, c), (b, c, a), (c, a, b)):
        u, v = q - p, r - p
        out.append(np.degrees(np.arccos(np.clip(u @ v / (np.linalg.norm(u) * np.linalg.norm(v)), -1, 1))))
    return out


def triangle_soup(seed, num_faces=NUM_FACES):
    """`num_faces` separate triangles in the box +-0.5: edge lengths in [0.01, 0.1] (the body mesh's scale), smallest angle
    >= 20 degrees (checked on the fp32 vertices).  -> vertices (3 F, 3) fp32, faces (F, 3) int32"""
    rng = np.random.default_rng(seed)
    verts = []
    while len(verts) < 3 * num_faces:
        a = rng.uniform(-0.5, 0.5, 3)
        d1, d2 = rng.standard_normal(3), rng.standard_normal(3)
        b = a + d1 / np.linalg.norm(d1) * rng.uniform(EDGE_MIN, EDGE_MAX)
        c = a + d2 / np.linalg.norm(d2) * rng.uniform(EDGE_MIN, EDGE_MAX)
        a, b, c = (p.astype(np.float32).astype(np.float64) for p in (a, b, c))
        edges = [np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c)]
        if min(edges) < EDGE_MIN or max(edges) > EDGE_MAX or min(_angles(a, b, c)) < ANGLE_MIN:
            continue
        verts += [a, b, c]
    return np.asarray(verts, np.float32), np.arange(3 * num_faces, dtype=np.int32).reshape(-1, 3)


def raw_quaternions(P, rng):
    """N(0,1) * U(0.2, 3): deliberately not unit"""
    return (rng.standard_normal((P, 4)) * rng.uniform(0.2, 3.0, (P, 1))).astype(np.float32)


def anchors(P, num_faces, rng):
    """mapping of P Gaussians: every face is used once P >= num_faces -> (face int32, uvw fp32, dist fp32)"""
    face = rng.permutation(np.arange(P) % num_faces).astype(np.int32)
    return face, rng.dirichlet((1.0, 1.0, 1.0), P).astype(np.float32), rng.uniform(-0.004, 0.004, P).astype(np.float32)


def displaced(vertices, faces, rng, share=0.3):
    """every vertex moved by up to `share` of its shortest incident edge, in a random direction -> fp32"""
    v = vertices.astype(np.float64)
    shortest = np.full(len(v), np.inf)
    for k in range(3):
        e = np.linalg.norm(v[faces[:, k]] - v[faces[:, (k + 1) % 3]], axis=1)
        np.minimum.at(shortest, faces[:, k], e)
        np.minimum.at(shortest, faces[:, (k + 1) % 3], e)
    d = rng.standard_normal(v.shape)
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, share, (len(v), 1)) * shortest[:, None]
    return (v + d).astype(np.float32)


def random_rotation(rng):
    """(3,3) float64, det +1, from a random unit quaternion"""
    q = rng.standard_normal((1, 4))
    return rotmat(q)[0]


def rigid(vertices, Rg, t):
    """v -> v Rg^T + t, computed in fp64, rounded to fp32 (what the kernel then reads)"""
    return (vertices.astype(np.float64) @ Rg.T + t).astype(np.float32)


def case(P, seed=None):
    """The inputs of one size: a soup, its displaced and its rigidly moved copy, P anchors and raw quaternions"""
    seed = 7000 + P if seed is None else seed
    rng = np.random.default_rng(seed)
    v, f = triangle_soup(seed)
    face, uvw, dist = anchors(P, len(f), rng)
    Rg, t = random_rotation(rng), rng.uniform(-0.3, 0.3, 3)
    return dict(P=P, vertices=v, faces=f, face=face, uvw=uvw, dist=dist, rot_raw=raw_quaternions(P, rng),
                posed=displaced(v, f, rng), Rg=Rg, t=t, moved=rigid(v, Rg, t))


DEGENERATE = ("repeated", "collinear", "nan", "inf")


def degenerate_case(where, seed=7700):
    """A soup of 40 sound faces plus four more (faces 40..43), which are the four degenerate kinds in the rest mesh, the
    posed mesh or both (`where` in "rest", "posed", "both"), and sound triangles otherwise.  Three Gaussians sit on every face.
    Also returns the all-sound pair of meshes: Gaussians on faces 0..39 must not notice the difference."""
    rng = np.random.default_rng(seed)
    v0, f0 = triangle_soup(seed)
    extra, _ = triangle_soup(seed + 1, num_faces=4)
    rest_sound = np.concatenate([v0, extra])
    faces = np.arange(len(rest_sound), dtype=np.int32).reshape(-1, 3)
    posed_sound = displaced(rest_sound, faces, rng)

    def spoil(v):
        v = v.copy()
        k = 3 * NUM_FACES
        v[k + 1] = v[k]                                                             # repeated vertex
        a, d = np.array([0.25, -0.125, 0.375], np.float32), np.array([3, 1, -2], np.float32) / 256
        v[k + 3], v[k + 4], v[k + 5] = a, a + d, a + 2 * d                           # collinear, exactly (few-bit numbers)
        v[k + 6, 1] = np.nan                                                        # NaN vertex
        v[k + 11, 0] = np.inf                                                       # Inf vertex
        return v
    rest = spoil(rest_sound) if where in ("rest", "both") else rest_sound
    posed = spoil(posed_sound) if where in ("posed", "both") else posed_sound
    P = 3 * len(faces)
    face = (np.arange(P) % len(faces)).astype(np.int32)
    return dict(P=P, faces=faces, face=face, uvw=rng.dirichlet((1.0, 1.0, 1.0), P).astype(np.float32),
                dist=rng.uniform(-0.004, 0.004, P).astype(np.float32), rot_raw=raw_quaternions(P, rng), rest=rest, posed=posed,
                rest_sound=rest_sound, posed_sound=posed_sound, bad=face >= NUM_FACES)


def matrix_error(q, R64):
    """largest element of |R(q) - R64|"""
    return float(np.abs(rotmat(q) - R64).max())


# ---------------------------------------------------------------------------------------------------- the end-to-end scene

SHEET_P, SHEET_HW = 200, 128
SHEET_AXIS_ANGLE = (np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.pi / 2)


def sheet_scene(seed=7800):
    """About 200 needle-shaped Gaussians (scales 10 : 1 : 1, SH degree 0, opacity 0.8) anchored on both sides of a small
    square sheet (5 x 5 quads in the plane x = 0, facing the camera of animation frame 0; every triangle once per winding), and the
    rigid motion of the test: 90 degrees about (1, 2, 3) / sqrt(14) through the origin, applied to the mesh and the camera."""
    rng = np.random.default_rng(seed)
    n, side = 5, 0.8
    g = np.linspace(-side / 2, side / 2, n + 1)
    vx, vz = np.meshgrid(g, g, indexing="ij")
    verts = np.stack([np.zeros(vx.size), vx.ravel(), vz.ravel()], 1).astype(np.float32)
    idx = lambda i, j: i * (n + 1) + j  # noqa: E731
    front = []
    for i in range(n):
        for j in range(n):
            front += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    front = np.asarray(front, np.int32)
    faces = np.concatenate([front, front[:, ::-1]]).astype(np.int32)
    P = SHEET_P
    face = rng.permutation(np.arange(P) % len(faces)).astype(np.int32)
    uvw = rng.dirichlet((1.0, 1.0, 1.0), P).astype(np.float32)
    dist = rng.uniform(0.002, 0.01, P).astype(np.float32)
    scaling = np.log(np.tile(np.array([[0.04, 0.004, 0.004]], np.float32), (P, 1))).astype(np.float32)
    axis, angle = SHEET_AXIS_ANGLE
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rg = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    from humangaussian_amd import synth
    c2w = np.asarray(synth.c2w_orbit(0.0, 0.0, 2.0), np.float64)
    M = np.eye(4)
    M[:3, :3] = Rg
    return dict(P=P, vertices=verts, faces=faces, face=face, uvw=uvw, dist=dist, rot_raw=raw_quaternions(P, rng),
                scaling=scaling, opacity=np.full((P, 1), np.log(0.8 / 0.2), np.float32),
                features_dc=rng.uniform(-1.5, 1.5, (P, 1, 3)).astype(np.float32), Rg=Rg, c2w=c2w, c2w_moved=M @ c2w,
                moved=rigid(verts, Rg, np.zeros(3)), fovy=np.radians(50.0), H=SHEET_HW, W=SHEET_HW)
