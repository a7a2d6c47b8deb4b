"""numpy restatement of the mesh view (include/hgs_rast.h: hgs_meshview_*; csrc/meshview.hip), the yardstick of
tests/test_mesh_view_cpu.py and tests/test_gpu_mesh_view.py.

Exact path: float32 arrays (numpy rounds every float32 operation once, as the library built with -ffp-contract=off does)
and int64 for the coverage.  The vertex stage also exists in float64 (`vertex_stage64`), to measure the fp32 stage's own
error.  Nothing here is fast: a Python loop over the faces, vectorised over each face's box of samples.
"""
import numpy as np

INVALID = np.int32(-2 ** 31)
f32 = np.float32
COORD_MAX = 2.0 ** 23
TILE = 16


# ---------------------------------------------------------------------------------------------------------- vertex stage
def vertex_stage32(vertices, mvp, H, W):
    """(xs, ys, zw, invw, valid) in float32, operation by operation as the header states them"""
    v = np.asarray(vertices, f32)
    m = np.asarray(mvp, f32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        c = [((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(4)]
        invw = f32(1.0) / c[3]
        xs = ((c[0] * invw) * f32(0.5) + f32(0.5)) * f32(W << 8)
        ys = ((c[1] * invw) * f32(0.5) + f32(0.5)) * f32(H << 8)
        zw = c[2] * invw
        valid = (c[3] > 0) & np.isfinite(xs) & np.isfinite(ys) & np.isfinite(zw) & (np.abs(xs) < COORD_MAX) & (np.abs(ys) < COORD_MAX)
    return xs, ys, zw, invw, valid


def vertex_records(vertices, mvp, H, W):
    """(V, 4) int32: {x_fix, y_fix, bits(zw), bits(invw)}, {INT32_MIN, 0, 0, 0} for an invalid vertex"""
    xs, ys, zw, invw, valid = vertex_stage32(vertices, mvp, H, W)
    rec = np.zeros((len(xs), 4), np.int32)
    rec[:, 0] = INVALID
    ok = np.nonzero(valid)[0]
    rec[ok, 0] = np.rint(xs[ok]).astype(np.int32)
    rec[ok, 1] = np.rint(ys[ok]).astype(np.int32)
    rec[ok, 2] = zw[ok].astype(f32).view(np.int32)
    rec[ok, 3] = invw[ok].astype(f32).view(np.int32)
    return rec


def vertex_stage64(vertices, mvp, H, W):
    """(xs, ys, zw, c3) in float64 from the same float32 inputs"""
    v = np.asarray(vertices, f32).astype(np.float64)
    m = np.asarray(mvp, f32).astype(np.float64)
    c = np.concatenate([v, np.ones((len(v), 1))], 1) @ m.T
    with np.errstate(all="ignore"):
        xs = (c[:, 0] / c[:, 3] * 0.5 + 0.5) * (W << 8)
        ys = (c[:, 1] / c[:, 3] * 0.5 + 0.5) * (H << 8)
        zw = c[:, 2] / c[:, 3]
    return xs, ys, zw, c[:, 3]


# ------------------------------------------------------------------------------------------------------------- coverage
def _cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def _owns(dx, dy):
    return dy > 0 or (dy == 0 and dx > 0)


def _face_setup(rec, face, V):
    """None for a dropped face, else (a, b, c, s, A) with int corners"""
    i0, i1, i2 = (int(i) for i in face)
    if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= V:
        return None
    a, b, c = ([int(t) for t in rec[i]] for i in (i0, i1, i2))
    if a[0] == int(INVALID) or b[0] == int(INVALID) or c[0] == int(INVALID):
        return None
    area2 = _cross(b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1])
    if area2 == 0:
        return None
    s = 1 if area2 > 0 else -1
    return a, b, c, s, s * area2


def _sample_box(a, b, c, H, W):
    """the pixels whose samples (c 256 + 128, r 256 + 128) lie in the corners' box, clipped to the image"""
    xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
    c0, c1 = max(-((128 - min(xs)) // 256), 0), min((max(xs) - 128) // 256, W - 1)      # ceil, floor
    r0, r1 = max(-((128 - min(ys)) // 256), 0), min((max(ys) - 128) // 256, H - 1)
    return c0, c1, r0, r1


def _edges(a, b, c, s, A, PX, PY):
    E0 = s * _cross(c[0] - b[0], c[1] - b[1], PX - b[0], PY - b[1])
    E1 = s * _cross(a[0] - c[0], a[1] - c[1], PX - c[0], PY - c[1])
    E2 = A - E0 - E1
    own = (_owns(s * (c[0] - b[0]), s * (c[1] - b[1])), _owns(s * (a[0] - c[0]), s * (a[1] - c[1])),
           _owns(s * (b[0] - a[0]), s * (b[1] - a[1])))
    inside = np.ones(E0.shape, bool)
    for E, o in zip((E0, E1, E2), own):
        inside &= (E > 0) | ((E == 0) & o)
    return E0, E1, E2, inside


def rasterize_records(rec, faces, H, W, return_counts=False):
    """rast (H, W, 4) float32 of one view from its vertex records [, the number of faces covering every sample]"""
    rec = np.asarray(rec, np.int32)
    faces = np.asarray(faces)
    V = len(rec)
    zw = rec[:, 2].copy().view(f32)
    iw = rec[:, 3].copy().view(f32)
    zbuf = np.full((H, W), np.inf, f32)
    idb = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    P = np.zeros((3, H, W), f32)
    counts = np.zeros((H, W), np.int64)
    for f, face in enumerate(faces):
        st = _face_setup(rec, face, V)
        if st is None:
            continue
        a, b, c, s, A = st
        c0, c1, r0, r1 = _sample_box(a, b, c, H, W)
        if c0 > c1 or r0 > r1:
            continue
        PX, PY = np.meshgrid(np.arange(c0, c1 + 1, dtype=np.int64) * 256 + 128, np.arange(r0, r1 + 1, dtype=np.int64) * 256 + 128)
        E0, E1, E2, inside = _edges(a, b, c, s, A, PX, PY)
        sub = (slice(r0, r1 + 1), slice(c0, c1 + 1))
        counts[sub] += inside
        ia = f32(1.0) / f32(A)
        b0, b1, b2 = E0.astype(f32) * ia, E1.astype(f32) * ia, E2.astype(f32) * ia
        i0, i1, i2 = (int(i) for i in face)
        with np.errstate(all="ignore"):
            z = (b0 * zw[i0] + b1 * zw[i1]) + b2 * zw[i2]
            ok = inside & (z >= -1) & (z <= 1)
            win = ok & ((z < zbuf[sub]) | ((z == zbuf[sub]) & (f < idb[sub])))
            zbuf[sub] = np.where(win, z, zbuf[sub])
            idb[sub] = np.where(win, f, idb[sub])
            for k, (bk, ik) in enumerate(((b0, i0), (b1, i1), (b2, i2))):
                P[k][sub] = np.where(win, bk * iw[ik], P[k][sub])
    hit = idb != np.iinfo(np.int64).max
    rast = np.zeros((H, W, 4), f32)
    with np.errstate(all="ignore"):
        d = (P[0] + P[1]) + P[2]
        rast[..., 0] = np.where(hit, P[0] / d, f32(0))
        rast[..., 1] = np.where(hit, P[1] / d, f32(0))
    rast[..., 2] = np.where(hit, zbuf, f32(0))
    rast[..., 3] = np.where(hit, (idb + 1).astype(f32), f32(0))
    return (rast, counts) if return_counts else rast


def tile_list_lengths(rec, faces, H, W):
    """(tiles_y, tiles_x): how many faces the library lists for every 16 x 16 tile (the tiles their sample box meets)"""
    rec = np.asarray(rec, np.int32)
    n = np.zeros(((H + TILE - 1) // TILE, (W + TILE - 1) // TILE), np.int64)
    for face in np.asarray(faces):
        st = _face_setup(rec, face, len(rec))
        if st is None:
            continue
        c0, c1, r0, r1 = _sample_box(st[0], st[1], st[2], H, W)
        if c0 <= c1 and r0 <= r1:
            n[r0 // TILE:r1 // TILE + 1, c0 // TILE:c1 // TILE + 1] += 1
    return n


# ---------------------------------------------------------------------------------------------------------- interpolate
def interpolate(attr, rast, faces):
    """attr (V, C), rast (H, W, 4) -> (H, W, C) float32; zeros where rast has no face"""
    attr = np.asarray(attr, f32)
    faces = np.asarray(faces)
    idf = rast[..., 3]
    hit = (idf >= 1) & (idf <= len(faces))
    fid = np.where(hit, idf, 1).astype(np.int64) - 1
    out = np.zeros(rast.shape[:2] + (attr.shape[1],), f32)
    if len(faces) == 0:
        return out
    u, v = rast[..., 0:1], rast[..., 1:2]
    a0, a1, a2 = (attr[faces[fid, k]] for k in range(3))
    with np.errstate(all="ignore"):
        val = ((u * a0) + (v * a1)) + (((f32(1.0) - u) - v) * a2)
    return np.where(hit[..., None], val, f32(0)).astype(f32)


def safe_normalise(n):
    """(..., 3) float32: (0, 0, 1) where dot <= 1e-20 (or NaN), else n / sqrt(max(dot, 1e-20))"""
    n = np.asarray(n, f32)
    with np.errstate(all="ignore"):
        dot = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        good = dot > f32(1e-20)
        ln = np.sqrt(np.maximum(dot, f32(1e-20)))
        out = n / ln[..., None]
    out = np.where(good[..., None], out, np.array([0, 0, 1], f32))
    return out.astype(f32)


def shade_normals(normals, rast, faces, background=1.0):
    """stage 6: interpolate, safe normalise, (n + 1) 0.5, background where no face"""
    n = safe_normalise(interpolate(normals, rast, faces))
    img = (n + f32(1.0)) * f32(0.5)
    return np.where((rast[..., 3:] > 0), img, f32(background)).astype(f32)


def shade_attributes(attr, rast, faces, background=0.0):
    img = interpolate(attr, rast, faces)
    return np.where((rast[..., 3:] > 0), img, f32(background)).astype(f32)


# ------------------------------------------------------------------------------------------------------- vertex normals
def csr_adjacency(faces, V):
    """(adj_start (V + 1,), adj (3 F,)): per vertex the entries 3 face + corner that name it, ascending"""
    flat = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    start = np.zeros(V + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(flat, minlength=V))
    return start.astype(np.int32), order.astype(np.int32)


def vertex_normals(vertices, faces, dtype=f32):
    """the unit vertex normals of stage 5 in `dtype`: float32 = the library's arithmetic, float64 = the yardstick (there
    the sum is normalised without the 1e-20 rule; callers compare only where float32 took the normal branch)"""
    v = np.asarray(vertices, f32).astype(dtype)
    faces = np.asarray(faces, np.int64)
    start, adj = csr_adjacency(faces, len(v))
    e1, e2 = v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
    fn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(dtype)
    n = np.zeros((len(v), 3), dtype)
    for i in range(len(v)):
        acc = np.zeros(3, dtype)
        for k in range(start[i], start[i + 1]):
            acc = acc + fn[adj[k] // 3]
        n[i] = acc
    if dtype == f32:
        return safe_normalise(n)
    with np.errstate(all="ignore"):
        return n / np.sqrt((n * n).sum(1))[:, None]


# --------------------------------------------------------------------------------------------------------------- scenes
def humanoid_views(H, W, azimuths=(0.0, 30.0, 200.0)):
    """the sampled views: synth.humanoid_mesh() through orbit_camera(10 deg, az, 1.6, 50 deg) -> (vertices, faces, mvps
    (B, 4, 4) float32, cams)"""
    from humangaussian_amd import synth
    v, f = synth.humanoid_mesh()
    cams = [synth.orbit_camera(10.0, az, 1.6, 50.0, H, W) for az in azimuths]
    mvps = np.stack([c.full_proj_transform.numpy().T for c in cams]).astype(f32)
    return v, f, mvps, cams


def triangle_soup(n=300, seed=0):
    """n random triangles in clip space with w = 1 (mvp = identity): mostly small, every tenth screen-sized, depths in
    (-1.2, 1.2) so that some fragments leave the depth range"""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(-1.1, 1.1, (n, 1, 2))
    size = np.where(np.arange(n) % 10 == 0, 2.5, rng.uniform(0.02, 0.5, n))[:, None, None]
    xy = ctr + size * rng.uniform(-1, 1, (n, 3, 2))
    z = rng.uniform(-1.2, 1.2, (n, 3, 1))
    v = np.concatenate([xy, z], 2).reshape(-1, 3).astype(f32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def ndc_of_pixel(p, size):
    """the NDC coordinate whose fixed-point image is exactly pixel coordinate p (in pixels, multiples of 1 / 256 up to 64
    are exact in float32 for power-of-two sizes; used with sizes 32 and 64)"""
    return f32(p / size * 2.0 - 1.0)


def stacked_quads(num_triangles, nearest, H=32, W=32):
    """num_triangles triangles over tile (1, 1) of a 32 x 32 image (mvp = identity): quads with corners at pixel coordinates 17 and 30 (they
    cover the samples of pixels 17 .. 29) at distinct depths, a last single triangle if the number is odd.  Layer k has depth 0.5 + k / 4096 except the layer at
    position `nearest` ('first', 'middle', 'last' in face order), which lies at 0.25."""
    layers = (num_triangles + 1) // 2
    near = {"first": 0, "middle": layers // 2, "last": layers - 1}[nearest]
    x0, x1 = ndc_of_pixel(17.0, W), ndc_of_pixel(30.0, W)
    y0, y1 = ndc_of_pixel(17.0, H), ndc_of_pixel(30.0, H)
    V, F = [], []
    for k in range(layers):
        z = 0.25 if k == near else 0.5 + k / 4096.0
        base = 4 * k
        V += [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
        F.append((base, base + 1, base + 2))
        if 2 * k + 1 < num_triangles:
            F.append((base, base + 2, base + 3))
    return np.asarray(V, f32), np.asarray(F, np.int32), near


def surface_cloud(vertices, faces, n=12000, seed=0):
    """n area-uniform points on the mesh (float32): the dense, opaque Gaussian cloud of the end-to-end test"""
    rng = np.random.default_rng(seed)
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    area = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    pick = rng.choice(len(f), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    w = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], 1)
    return (w[:, :, None] * v[f[pick]]).sum(1).astype(f32)


CLOUD_SCALE, CLOUD_OPACITY = 0.01, 0.99
