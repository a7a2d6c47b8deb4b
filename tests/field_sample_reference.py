"""numpy restatement of the field at arbitrary points (include/hgs_rast.h: hgs_fsample), the yardstick of
tests/test_field_sample_cpu.py and tests/test_gpu_field_sample.py.  Written from the definition, not from the kernels, on
top of fields_reference.prepare / inverse_coefficients:

  sample(cloud, points, ..., dtype=np.float64)   everything in fp64 from the fp32 inputs, the block of a point included
  sample(cloud, points, ..., dtype=np.float32)   fp32 with the reference's own Sigma^-1 (the adjugate) and sequential sums
                                                 (np.add.accumulate): what the same formulas lose in fp32

`near` flags the points within NEAR (normalised units) of a plane between two blocks, axis[b * split] for 0 < b < nb: after
the fp32 normalisation of a world coordinate such a point may fall in either block, so the two sides need not have summed
the same list.  Points given in normalised coordinates are used untouched, the comparisons of fp32 numbers are exact in
fp64, and membership is the same on both sides: the flag is not needed there."""
import numpy as np

import fields_reference as FR

NEAR = 1e-6


class Sampled:
    pass


def cells(axis, n):
    """(number of samples <= n) - 1, clamped to [0, R - 1], per coordinate."""
    return np.clip(np.searchsorted(axis, n, side="right") - 1, 0, len(axis) - 1)


def normalise(points, P, dtype, normalized):
    q = np.asarray(points, np.float32)
    if normalized:
        return q.astype(dtype)
    if dtype == np.float32:
        return (q - P.center.astype(np.float32)) * np.float32(P.scale)
    return (q.astype(np.float64) - P.center) * P.scale


def sample(cloud, points, colors=None, resolution=128, num_blocks=16, relax_ratio=1.5, dtype=np.float64, normalized=False,
           prepared=None, chunk=512):
    """Sampled with density (M,), G (M,3), normal (M,3), color (M,3) or None, block (M,3), finite (M,), near (M,), n (M,3).
    `colors` (P,3) is indexed by the original Gaussian index."""
    P = prepared or FR.prepare(*cloud, resolution, num_blocks, relax_ratio, dtype)
    M = len(points)
    out = Sampled()
    out.prepared = P
    with np.errstate(invalid="ignore", over="ignore"):
        n = normalise(points, P, dtype, normalized)
    out.n = n
    out.finite = np.isfinite(n).all(1)
    axis = P.axis.astype(dtype)
    nf = np.where(out.finite[:, None], n, dtype(0))
    out.block = np.stack([cells(axis, nf[:, a]) for a in range(3)], 1) // P.split
    planes = P.axis[np.arange(1, num_blocks) * P.split].astype(np.float64)
    out.near = out.finite & (np.abs(nf.astype(np.float64)[:, :, None] - planes[None, None, :]) < NEAR).any((1, 2))
    out.density, out.G = np.zeros(M, dtype), np.zeros((M, 3), dtype)
    csum = np.zeros((M, 3), dtype)
    if len(P.n):
        co = FR.inverse_coefficients(P, dtype)
        kept_colors = None if colors is None else np.asarray(colors, np.float32)[P.index].astype(dtype)
        flat = (out.block[:, 0] * num_blocks + out.block[:, 1]) * num_blocks + out.block[:, 2]
        flat = np.where(out.finite, flat, -1)
        total = (lambda t: np.add.accumulate(t, axis=1)[:, -1]) if dtype == np.float32 else (lambda t: t.sum(1))
        half = dtype(0.5)
        for b in np.unique(flat[flat >= 0]):
            bx, by, bz = b // (num_blocks * num_blocks), b // num_blocks % num_blocks, b % num_blocks
            g = np.nonzero(P.inside[0][:, bx] & P.inside[1][:, by] & P.inside[2][:, bz])[0]        # ascending index
            if len(g) == 0:
                continue
            pts = np.nonzero(flat == b)[0]
            c = co[g]
            for p0 in range(0, len(pts), chunk):
                pp = pts[p0:p0 + chunk]
                d = nf[pp][:, None, :] - P.n[g][None]
                x, y, z = d[..., 0], d[..., 1], d[..., 2]
                with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                    power = (-half * (x * x * c[:, 0] + y * y * c[:, 3] + z * z * c[:, 5]) - x * y * c[:, 1]
                             - x * z * c[:, 2] - y * z * c[:, 4])
                    w = P.opacity[g] * np.where(power > 0, dtype(0), np.exp(np.minimum(power, dtype(0))))
                    out.density[pp] = total(w)
                    out.G[pp, 0] = total(w * (c[:, 0] * x + c[:, 1] * y + c[:, 2] * z))
                    out.G[pp, 1] = total(w * (c[:, 1] * x + c[:, 3] * y + c[:, 4] * z))
                    out.G[pp, 2] = total(w * (c[:, 2] * x + c[:, 4] * y + c[:, 5] * z))
                    if kept_colors is not None:
                        for k in range(3):
                            csum[pp, k] = total(w * kept_colors[g, k])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.abs(out.G).max(1)                                  # |G| of G scaled by its largest component, as defined
        ok = (m > 0) & np.isfinite(out.G).all(1)
        u = out.G / np.where(ok, m, 1)[:, None]
        out.normal = np.where(ok[:, None], u / np.sqrt((u * u).sum(1))[:, None], dtype(0)).astype(dtype)
        out.color = None
        if colors is not None:
            has = out.density != 0
            out.color = np.where(has[:, None], csum / np.where(has, out.density, 1)[:, None], dtype(0)).astype(dtype)
    return out


def angles(a, b):
    """Angle between corresponding rows, accurate for small angles: atan2(|a x b|, a . b) in fp64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))


def errors(got, ref):
    """(density relative distance, density absolute distance below the floor, colour absolute error or None, normal angle
    error) of one Sampled-like triple against the fp64 restatement `ref`, over the floors of the gates: colour where the
    density exceeds 1e-3 of its maximum, normals where |G| is at least 1e-3 of its maximum."""
    density, normal, color = got
    rel, ab = FR.distance(density, ref.density)
    dens_ok = ref.density > 1e-3 * ref.density.max() if len(ref.density) else np.zeros(0, bool)
    gn = np.linalg.norm(ref.G, axis=1)
    g_ok = gn >= 1e-3 * gn.max() if len(gn) and gn.max() > 0 else np.zeros(len(gn), bool)
    ce = None
    if color is not None and ref.color is not None:
        ce = float(np.abs(np.asarray(color, np.float64) - ref.color)[dens_ok].max()) if dens_ok.any() else 0.0
    ne = float(angles(np.asarray(normal)[g_ok], ref.normal[g_ok]).max()) if g_ok.any() else 0.0
    return rel, ab, ce, ne


def subset(s, keep):
    """The rows `keep` of a Sampled (the arrays the gates read)."""
    out = Sampled()
    out.density, out.G, out.normal = s.density[keep], s.G[keep], s.normal[keep]
    out.color = None if s.color is None else s.color[keep]
    return out


def face_agreement(vertices, faces, normals):
    """Share of the faces whose normal (b - a) x (c - a) has a positive dot product with the sum of its three vertex normals."""
    v, f, n = np.asarray(vertices, np.float64), np.asarray(faces, np.int64), np.asarray(normals, np.float64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return float(((fn * (n[f[:, 0]] + n[f[:, 1]] + n[f[:, 2]])).sum(1) > 0).mean())
