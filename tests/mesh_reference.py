"""fp64 numpy reference of the mesh queries of csrc/mesh.hip (include/hgs_rast.h, hgs_mesh_query) and the procedural test
meshes.  Brute force over all faces:
  - closest point: Ericson's region-based closest point on every triangle, (d2, face) lexicographic; also the runner-up's
    d2, so a test can tell a clear winner from a near tie;
  - ray stab: the same 64 rays +-d_i (32 Fibonacci-lattice directions), inside iff all of them hit a face at t > 0;
  - winding number (solid angles, Van Oosterom-Strackee): the inside test of a closed mesh, to check the ray stab against.
Faces whose fp32 cross product is exactly zero are skipped, as on the device."""
import math

import numpy as np

# ------------------------------------------------------------------------------------------------ meshes


def icosphere(subdiv=5, radius=1.0):
    """(V,3) float32, (F,3) int32, outward winding; 20 * 4^subdiv faces (20,480 at 5)."""
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def cube(half=0.5):
    """The axis-aligned cube [-half, half]^3: 8 vertices, 12 faces, outward winding."""
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, c, d in quads:
        f += [(a, b, c), (a, c, d)]
    f = np.array(f, np.int32)
    if signed_volume(v, f) < 0:
        f = f[:, ::-1].copy()
    return v, f


def torus(R=0.6, r=0.25, n_major=48, n_minor=24):
    """Closed torus around the z axis, outward winding."""
    u = np.linspace(0, 2 * np.pi, n_major, endpoint=False)
    w = np.linspace(0, 2 * np.pi, n_minor, endpoint=False)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(ww)) * np.cos(uu), (R + r * np.cos(ww)) * np.sin(uu), r * np.sin(ww)], -1).reshape(-1, 3)
    f = []
    for i in range(n_major):
        for j in range(n_minor):
            a, b = i * n_minor + j, ((i + 1) % n_major) * n_minor + j
            c, d = ((i + 1) % n_major) * n_minor + (j + 1) % n_minor, i * n_minor + (j + 1) % n_minor
            f += [(a, b, c), (a, c, d)]
    f = np.array(f, np.int32)
    if signed_volume(v, f) < 0:
        f = f[:, ::-1].copy()
    return v.astype(np.float32), f


def signed_volume(v, f):
    v = np.asarray(v, np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def face_normals(v, f):
    v = np.asarray(v, np.float64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return n / (np.linalg.norm(n, axis=1, keepdims=True) + 1e-300)


def valid_faces(v, f):
    """The device's skip rule: fp32 cross(v1 - v0, v2 - v0) exactly zero (or not finite)."""
    v32 = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        e1, e2 = v32[f[:, 1]] - v32[f[:, 0]], v32[f[:, 2]] - v32[f[:, 0]]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(np.float32)
    return np.any(n != 0, axis=1) & np.all(np.isfinite(n), axis=1)


# ------------------------------------------------------------------------------------------------ closest point


def closest_on_tris(p, a, b, c):
    """Ericson's closest point of p (..., 3) on triangles (a, b, c) (..., 3), broadcast: (d2, v, w)."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        den = va + vb + vc
        v = np.where(den != 0, vb / den, 0.0)
        w = np.where(den != 0, vc / den, 0.0)
        e_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        e_ac = d2 / (d2 - d6)
        e_ab = d1 / (d1 - d3)
    r_bc = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
    v, w = np.where(r_bc, 1 - e_bc, v), np.where(r_bc, e_bc, w)
    r_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    v, w = np.where(r_ac, 0.0, v), np.where(r_ac, e_ac, w)
    r_c = (d6 >= 0) & (d5 <= d6)
    v, w = np.where(r_c, 0.0, v), np.where(r_c, 1.0, w)
    r_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    v, w = np.where(r_ab, e_ab, v), np.where(r_ab, 0.0, w)
    r_b = (d3 >= 0) & (d4 <= d3)
    v, w = np.where(r_b, 1.0, v), np.where(r_b, 0.0, w)
    r_a = (d1 <= 0) & (d2 <= 0)
    v, w = np.where(r_a, 0.0, v), np.where(r_a, 0.0, w)
    q = a + ab * v[..., None] + ac * w[..., None]
    d = p - q
    return (d * d).sum(-1), v, w


def closest_point(points, v, f, chunk=64):
    """fp64 brute force: (d2, face, uvw, runner-up d2) per point; face -1 / NaN for non-finite points."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    v64 = np.asarray(v, np.float64)
    ok = valid_faces(v, f)
    fi = np.nonzero(ok)[0]
    a, b, c = v64[f[fi, 0]], v64[f[fi, 1]], v64[f[fi, 2]]
    P = len(pts)
    d2o, fo, uvwo, d2b = np.full(P, np.nan), np.full(P, -1, np.int64), np.zeros((P, 3)), np.full(P, np.inf)
    fin = np.all(np.isfinite(pts), axis=1)
    idx = np.nonzero(fin)[0]
    for s in range(0, len(idx), chunk):
        ii = idx[s:s + chunk]
        d2, vv, ww = closest_on_tris(pts[ii, None, :], a[None], b[None], c[None])
        k = np.argmin(d2, axis=1)                       # first minimum = lowest face index among ties
        r = np.arange(len(ii))
        d2o[ii], fo[ii] = d2[r, k], fi[k]
        uvwo[ii] = np.stack([1 - vv[r, k] - ww[r, k], vv[r, k], ww[r, k]], 1)
        if d2.shape[1] > 1:
            d2[r, k] = np.inf
            d2b[ii] = d2.min(axis=1)
    return d2o, fo, uvwo, d2b


# ------------------------------------------------------------------------------------------------ sign


def ray_dirs():
    """The 32 fixed directions (fp64): z_i = 1 - (2i + 1) / 32, theta_i = 2 pi frac(0.6180339887 i + 0.1234)."""
    i = np.arange(32, dtype=np.float64)
    z = 1.0 - (2 * i + 1) / 32.0
    fr = 0.6180339887 * i + 0.1234
    th = 2 * math.pi * (fr - np.floor(fr))
    r = np.sqrt(1 - z * z)
    return np.stack([r * np.cos(th), r * np.sin(th), z], 1)


def raystab_inside(points, v, f, chunk=256):
    """fp64 ray stab: inside iff all 64 rays +-d_i hit a (non-skipped) face at t > 0 (Moeller-Trumbore, inclusive edges).
    Per direction the three numerators are affine in the point: three (P, F) matrix products."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    v64 = np.asarray(v, np.float64)
    ff = f[valid_faces(v, f)]
    v0, e1, e2 = v64[ff[:, 0]], v64[ff[:, 1]] - v64[ff[:, 0]], v64[ff[:, 2]] - v64[ff[:, 0]]
    n = np.cross(e1, e2)
    inside = np.all(np.isfinite(pts), axis=1)
    for d in ray_dirs():
        pv = np.cross(d, e2)                           # u = (p - v0) . pv / det
        rv = np.cross(e1, d)                           # v = (p - v0) . rv / det   (= d . ((p - v0) x e1) / det)
        det = (e1 * pv).sum(1)
        nz = det != 0
        for s in range(0, len(pts), chunk):
            live = np.nonzero(inside[s:s + chunk])[0] + s
            if len(live) == 0:
                continue
            p = pts[live]
            un = p @ pv.T - (v0 * pv).sum(1)
            vn = p @ rv.T - (v0 * rv).sum(1)
            tn = p @ n.T - (v0 * n).sum(1)             # t = e2 . ((p - v0) x e1) / det = (p - v0) . n / det
            sg = np.sign(det)
            u_, v_, t_ = un * sg, vn * sg, tn * sg     # scaled by |det|: barycentrics u_, v_ >= 0, u_ + v_ <= |det|
            hit_tri = nz & (u_ >= 0) & (v_ >= 0) & (u_ + v_ <= np.abs(det))
            hit_fwd = np.any(hit_tri & (t_ > 0), axis=1)
            hit_bwd = np.any(hit_tri & (t_ < 0), axis=1)
            inside[live] = hit_fwd & hit_bwd
    return inside


def winding_number(points, v, f, chunk=128):
    """Generalised winding number (solid angle / 4 pi) of each point; ~1 inside, ~0 outside a closed outward mesh."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    v64 = np.asarray(v, np.float64)
    A, B, C = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    out = np.zeros(len(pts))
    for s in range(0, len(pts), chunk):
        p = pts[s:s + chunk, None, :]
        a, b, c = A[None] - p, B[None] - p, C[None] - p
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + chunk] = (2 * np.arctan2(num, den)).sum(1) / (4 * math.pi)
    return out
