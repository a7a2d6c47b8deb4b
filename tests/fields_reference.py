"""numpy restatement of the density field and of marching cubes (include/hgs_rast.h: hgs_field_*, hgs_mc_*), the yardstick
of tests/test_fields_cpu.py and tests/test_gpu_fields.py.  Written from the definition, not from the kernels:

  field(..., dtype=np.float64)                the field in fp64 from the fp32 inputs (Sigma^-1 by numpy.linalg.inv)
  field(..., dtype=np.float32)                the reference's own arithmetic in fp32: Sigma = (R S)(R S)^T, the adjugate
                                              with 1 / (det + 1e-24), power as the reference spells it
  marching_cubes(field, thr)                  per cell, no vertex sharing: a triangle soup (T, 3, 3) in fp64
"""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPACITY_CUT = np.float32(0.005)
NEAR = 1e-6          # a Gaussian this close (normalised units) to a cut plane may fall on either side in fp32


def axis_samples(resolution):
    """The reference's sample positions: torch.linspace(-1, 1, resolution) in fp32."""
    return torch.linspace(-1, 1, resolution).numpy().copy()


def rotation_matrices(q):
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3), q.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


class Prepared:
    pass


def prepare(xyz, opacity, scaling, rotation, resolution, num_blocks, relax_ratio, dtype):
    """Steps 1-4 of the definition: the kept Gaussians, normalised, and which blocks list them."""
    xyz, opacity, scaling, rotation = (np.asarray(a, np.float32) for a in (xyz, opacity.reshape(-1), scaling, rotation))
    keep = (opacity > OPACITY_CUT) & np.isfinite(xyz).all(1)
    P = Prepared()
    P.keep, P.index = keep, np.nonzero(keep)[0]
    P.resolution, P.num_blocks, P.split = resolution, num_blocks, resolution // num_blocks
    P.axis = axis_samples(resolution)
    grow = np.float32((2 / num_blocks) * relax_ratio)
    first = P.axis[np.arange(num_blocks) * P.split]
    last = P.axis[np.arange(num_blocks) * P.split + P.split - 1]
    P.lo, P.hi = (first - grow).astype(np.float32), (last + grow).astype(np.float32)     # fp32 arithmetic, as the reference
    if not keep.any():
        P.center, P.scale, P.n = np.zeros(3, np.float32), 1.0, np.zeros((0, 3), dtype)
        P.inside = [np.zeros((0, num_blocks), bool)] * 3
        P.near = P.inside
        return P
    x, s, q = xyz[keep], scaling[keep], rotation[keep]
    mn, mx = x.min(0), x.max(0)
    if dtype == np.float32:
        P.center = (mn + mx) / np.float32(2)
        P.scale = 1.8 / float((mx - mn).max())                       # a Python float, as the reference's .item()
        sc = np.float32(P.scale)
        P.n, P.s, P.q = (x - P.center) * sc, s * sc, q
    else:
        P.center = (mn.astype(np.float64) + mx.astype(np.float64)) / 2
        P.scale = 1.8 / float((mx.astype(np.float64) - mn.astype(np.float64)).max())
        P.n, P.s, P.q = (x.astype(np.float64) - P.center) * P.scale, s.astype(np.float64) * P.scale, q.astype(np.float64)
    P.opacity = opacity[keep].astype(dtype)
    with np.errstate(invalid="ignore"):
        P.inside = [(P.n[:, a, None] > P.lo[None, :]) & (P.n[:, a, None] < P.hi[None, :]) for a in range(3)]
        P.near = [(np.abs(P.n[:, a, None] - P.lo[None, :].astype(np.float64)) < NEAR) |
                  (np.abs(P.n[:, a, None] - P.hi[None, :].astype(np.float64)) < NEAR) for a in range(3)]
    return P


def _count(m0, m1, m2):
    nb = m0.shape[1]
    out = np.zeros((nb * nb, nb), np.int64)
    for g0 in range(0, len(m0), 16384):
        sl = slice(g0, g0 + 16384)
        xy = (m0[sl, :, None] & m1[sl, None, :]).reshape(-1, nb * nb).astype(np.float32)
        out += np.rint(xy.T @ m2[sl].astype(np.float32)).astype(np.int64)
    return out.reshape(nb, nb, nb)


def block_counts(P):
    """((nb,)*3 list lengths, (nb,)*3 bool: the block holds a Gaussian within NEAR of one of its cut planes)."""
    counts = _count(*P.inside)
    maybe = [i | n for i, n in zip(P.inside, P.near)]
    sure = [i & ~n for i, n in zip(P.inside, P.near)]
    return counts, _count(*maybe) != _count(*sure)


def inverse_coefficients(P, dtype):
    """(K, 6) xx, xy, xz, yy, yz, zz of Sigma^-1."""
    R = rotation_matrices(P.q)
    if dtype == np.float64:
        S = np.einsum("gik,gk,gjk->gij", R, P.s * P.s, R)
        inv = np.linalg.inv(S)
        return np.stack([inv[:, 0, 0], inv[:, 0, 1], inv[:, 0, 2], inv[:, 1, 1], inv[:, 1, 2], inv[:, 2, 2]], 1)
    L = (R * P.s[:, None, :]).astype(np.float32)                     # R @ diag(s)
    S = np.matmul(L, L.transpose(0, 2, 1)).astype(np.float32)
    a, b, c, d, e, f = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    inv_det = np.float32(1) / (a * d * f + np.float32(2) * e * c * b - e ** 2 * a - c ** 2 * d - b ** 2 * f + np.float32(1e-24))
    return np.stack([(d * f - e ** 2) * inv_det, (e * c - b * f) * inv_det, (e * b - c * d) * inv_det,
                     (a * f - c ** 2) * inv_det, (b * c - e * a) * inv_det, (a * d - b ** 2) * inv_det], 1).astype(np.float32)


def field(xyz, opacity, scaling, rotation, resolution=128, num_blocks=16, relax_ratio=1.5, dtype=np.float64, prepared=None):
    """(occ (R,R,R) dtype, Prepared).  Sum order inside a block: ascending Gaussian index, numpy's pairwise summation."""
    P = prepared or prepare(xyz, opacity, scaling, rotation, resolution, num_blocks, relax_ratio, dtype)
    occ = np.zeros((resolution,) * 3, dtype)
    if len(P.n) == 0:
        return occ, P
    co = inverse_coefficients(P, dtype)
    ax, s = P.axis.astype(dtype), P.split
    half = dtype(0.5)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for bx in np.nonzero(P.inside[0].any(0))[0]:
            mx_ = P.inside[0][:, bx]
            for by in np.nonzero((P.inside[1] & mx_[:, None]).any(0))[0]:
                mxy = mx_ & P.inside[1][:, by]
                for bz in np.nonzero((P.inside[2] & mxy[:, None]).any(0))[0]:
                    g = np.nonzero(mxy & P.inside[2][:, bz])[0]
                    xs, ys, zs = ax[bx * s:(bx + 1) * s], ax[by * s:(by + 1) * s], ax[bz * s:(bz + 1) * s]
                    val = np.zeros((s, s, s), dtype)
                    for g0 in range(0, len(g), 1024):                # the reference's batches of 1024 Gaussians
                        gg = g[g0:g0 + 1024]
                        x = xs[:, None, None, None] - P.n[gg, 0]
                        y = ys[None, :, None, None] - P.n[gg, 1]
                        z = zs[None, None, :, None] - P.n[gg, 2]
                        c = co[gg]
                        power = (-half * (x * x * c[:, 0] + y * y * c[:, 3] + z * z * c[:, 5]) - x * y * c[:, 1]
                                 - x * z * c[:, 2] - y * z * c[:, 4])
                        w = np.where(power > 0, dtype(0), np.exp(np.minimum(power, dtype(0))))
                        val += (P.opacity[gg] * w).sum(-1)
                    occ[bx * s:(bx + 1) * s, by * s:(by + 1) * s, bz * s:(bz + 1) * s] = val
    return occ, P


def distance(got, ref, rel_floor=1e-3):
    """(largest relative distance over the samples above rel_floor * max, largest absolute distance over the others)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    big = ref > rel_floor * ref.max()
    d = np.abs(got - ref)
    return float((d[big] / ref[big]).max()) if big.any() else 0.0, float(d[~big].max()) if (~big).any() else 0.0


# ------------------------------------------------------------------------------------------------ marching cubes

CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])


def load_table():
    """(tri (256, 16) int, edge corners (12, 2) int) parsed from the header the kernels compile."""
    src = open(os.path.join(ROOT, "humangaussian_amd", "csrc", "mc_table.h")).read()
    body = src[src.index("HGS_MC_EDGE_CORNERS[12][2]"):]
    edges = np.array([int(v) for v in re.findall(r"-?\d+", body[body.index("=") :body.index(";")])]).reshape(12, 2)
    body = src[src.index("HGS_MC_TRI_TABLE[256][HGS_MC_ROW]"):]
    tri = np.array([int(v) for v in re.findall(r"-?\d+", body[body.index("=") :body.index("};")])]).reshape(256, 16)
    return tri, edges


def cell_cases(f, thr):
    inside = np.asarray(f) >= thr
    X, Y, Z = inside.shape
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int32)
    for i, (cx, cy, cz) in enumerate(CORNERS):
        case |= inside[cx:cx + X - 1, cy:cy + Y - 1, cz:cz + Z - 1].astype(np.int32) << i
    return case


def marching_cubes(f, thr):
    """Triangle soup (T, 3, 3) fp64, index coordinates; each corner of a triangle interpolated on its own."""
    f = np.asarray(f, np.float64)
    tri, edges = load_table()
    case = cell_cases(f, thr)
    out = []
    for c in np.unique(case):
        row = tri[c]
        nt = int((row >= 0).sum()) // 3
        if nt == 0:
            continue
        cells = np.argwhere(case == c)                                  # (n, 3)
        verts = np.empty((len(cells), nt * 3, 3))
        for k in range(nt * 3):
            a, b = edges[row[k]]
            pa, pb = cells + CORNERS[a], cells + CORNERS[b]
            fa, fb = f[pa[:, 0], pa[:, 1], pa[:, 2]], f[pb[:, 0], pb[:, 1], pb[:, 2]]
            t = (thr - fa) / (fb - fa)
            verts[:, k] = pa + (pb - pa) * t[:, None]
        out.append(verts.reshape(-1, 3, 3))
    return np.concatenate(out) if out else np.zeros((0, 3, 3))


def weld(soup, decimals=6):
    """(vertices (V,3), faces (T,3)): corners that agree after rounding become one vertex."""
    if len(soup) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    v, inv = np.unique(np.round(soup.reshape(-1, 3), decimals), axis=0, return_inverse=True)
    return v, inv.reshape(-1, 3)


def edge_use(faces):
    """Undirected edges of the faces and how many faces use each."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(np.sort(e, 1), axis=0, return_counts=True)


def is_closed(faces):
    return len(faces) > 0 and bool((edge_use(faces)[1] == 2).all())


def is_oriented(faces):
    """Every directed edge occurs once, and so does its opposite: a consistently wound closed surface."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    u, n = np.unique(e, axis=0, return_counts=True)
    return bool((n == 1).all()) and {tuple(r) for r in u} == {(b, a) for a, b in u}


def euler(vertices, faces):
    used = len(np.unique(np.asarray(faces)))
    return used - len(edge_use(faces)[0]) + len(faces)


def signed_volume(v, f):
    v = np.asarray(v, np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------------------------------------ test clouds

def cloud(n, seed, radii=(0.25, 0.15, 0.75), scale0=0.02, spread=0.6, surface=True):
    """The cloud of the issue's fixture: points on an ellipsoid, scales scale0 * exp(spread * N), random quaternions,
    opacities 0.002 + 0.95 U."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if not surface:
        d *= rng.uniform(0, 1, (n, 1)) ** (1 / 3)
    xyz = (d * np.asarray(radii)).astype(np.float32)
    scaling = (scale0 * np.exp(spread * rng.normal(size=(n, 3)))).astype(np.float32)
    rotation = rng.normal(size=(n, 4)).astype(np.float32)
    opacity = (0.002 + 0.95 * rng.uniform(size=(n, 1))).astype(np.float32)
    return xyz, opacity, scaling, rotation
