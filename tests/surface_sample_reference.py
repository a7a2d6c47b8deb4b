"""numpy restatement of the surface sampler's definition (include/hgs_rast.h: hgs_surface_cdf / hgs_surface_sample), the
case table of tests/test_gpu_surface_sample.py and, per sample, how far its table look-up is from a table boundary.

The device sums the fp64 areas in its own fixed order and numpy in `np.cumsum`'s: the two tables may differ in their last
bits.  A sample whose `t` lies farther from every boundary than those bits can reach gets the same face from both; the
cases are chosen (and test_surface_sample_cpu.py checks) so that EVERY sample of every case does, which is what lets the
GPU test demand exact faces of all samples."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) of 32-bit words -> (..., 4) words; uint64 arithmetic throughout"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                       # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack(c, -1).astype(np.uint32)


def words(n, seed=0, offset=0):
    """(n, 4) uint32: the four words of samples offset .. offset + n - 1"""
    g = (np.arange(n, dtype=np.uint64) + np.uint64(offset))             # wraps at 2^64 like the device
    z = np.zeros(n, np.uint64)
    ctr = np.stack([g & MASK, g >> S32, z, z], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64), (n, 2))
    return philox4x32_10(ctr, key)


def face_areas(vertices, faces):
    """fp64 areas from the fp32 vertices; 0 for a non-finite area and for a face with an index outside [0, V)"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    ok = ((f >= 0) & (f < len(v))).all(1)
    fs = np.where(ok[:, None], f, 0)
    if len(v) == 0:
        return np.zeros(len(f))
    a, b, c = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
    e1, e2 = b - a, c - a
    with np.errstate(all="ignore"):
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.where(ok & np.isfinite(area), area, 0.0)


def sample(vertices, faces, n, seed=0, offset=0):
    """-> dict: face (n,) int64, uvw (n,3) fp32, points (n,3) fp32 in the kernel's operation order, points64 (n,3) the same
    expression in fp64, cdf (F,) fp64, area, num_positive, margin (n,) = |t - nearest table boundary| / A"""
    v32 = np.asarray(vertices, np.float32)
    f = np.asarray(faces).astype(np.int64)
    F = len(f)
    area = face_areas(v32, f)
    cdf = np.cumsum(area)
    A = float(cdf[-1])
    x = words(n, seed, offset)
    u = ((x[:, 0] >> np.uint32(5)).astype(np.float64) * 67108864.0 + (x[:, 1] >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53
    t = u * A
    face = np.minimum(np.searchsorted(cdf, t, side="right"), F - 1).astype(np.int64)
    k1, k2 = (x[:, 2] >> np.uint32(8)).astype(np.int64), (x[:, 3] >> np.uint32(8)).astype(np.int64)
    fold = k1 + k2 > 1 << 24
    k1, k2 = np.where(fold, (1 << 24) - k1, k1), np.where(fold, (1 << 24) - k2, k2)
    uvw = (np.stack([(1 << 24) - k1 - k2, k1, k2], -1).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    a, b, c = (v32[f[face, j]] for j in range(3))
    w = uvw
    points = (a * w[:, 0:1] + b * w[:, 1:2]) + c * w[:, 2:3]                    # fp32 products and sums, in this order
    a64, b64, c64, w64 = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64), w.astype(np.float64)
    points64 = (a64 * w64[:, 0:1] + b64 * w64[:, 1:2]) + c64 * w64[:, 2:3]
    # distance of t to the nearest boundary that separates two different answers (the distinct table values below A)
    edges = np.unique(cdf[:-1]) if F > 1 else np.zeros(0)
    if len(edges) and n:
        j = np.searchsorted(edges, t)
        lo = np.abs(t - edges[np.clip(j - 1, 0, len(edges) - 1)])
        hi = np.abs(edges[np.clip(j, 0, len(edges) - 1)] - t)
        margin = np.minimum(lo, hi) / A
    else:
        margin = np.full(n, np.inf)
    return dict(face=face, uvw=uvw, points=points, points64=points64, cdf=cdf, area=A,
                num_positive=int((area > 0).sum()), margin=margin)


# ---- the cases of the GPU test ----------------------------------------------------------------------------------------
SAMPLE_SEED = 7
FACE_COUNTS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049)
SAMPLE_COUNTS = (0, 1, 255, 256, 257, 1000)
VARIANTS = ("plain", "zero_area", "one_huge", "nan_vertex", "bad_index")


def soup(F, variant="plain"):
    """A triangle soup of F faces, vertices uniform in [-1, 1]^3, mesh seed 1000 + F -> (vertices (3F,3) fp32, faces (F,3) int32)
      zero_area   faces 0, F/2 and F-1 collapsed (their third vertex repeats their first)
      one_huge    face F/3 scaled about its first vertex to 10^8 times the area of an average face
      nan_vertex  one vertex of face F/2 is NaN            bad_index  face F/2 names vertex V"""
    rng = np.random.default_rng(1000 + F)
    v = rng.uniform(-1.0, 1.0, (3 * F, 3)).astype(np.float32)
    f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    if variant == "zero_area":
        for k in (0, F // 2, F - 1):
            v[3 * k + 2] = v[3 * k]
    elif variant == "one_huge":
        k = F // 3
        mean = face_areas(v, f).mean()
        s = np.float32(np.sqrt(1e8 * mean / face_areas(v, f)[k]))
        v[3 * k + 1] = v[3 * k] + s * (v[3 * k + 1] - v[3 * k])
        v[3 * k + 2] = v[3 * k] + s * (v[3 * k + 2] - v[3 * k])
    elif variant == "nan_vertex":
        v[3 * (F // 2) + 1, 1] = np.nan
    elif variant == "bad_index":
        f[F // 2, 2] = 3 * F
    elif variant != "plain":
        raise ValueError(variant)
    return v, f


def cases():
    """(name, F, variant, N) of every GPU case"""
    out = []
    for F in FACE_COUNTS:
        for N in SAMPLE_COUNTS:
            out.append((f"F{F}-N{N}", F, "plain", N))
        if F >= 63:
            out.append((f"F{F}-zero_area", F, "zero_area", 1000))
            out.append((f"F{F}-one_huge", F, "one_huge", 1000))
    out.append(("F1025-nan_vertex", 1025, "nan_vertex", 1000))
    out.append(("F1025-bad_index", 1025, "bad_index", 1000))
    out.append(("F20908-N100000", 20908, "plain", 100000))
    # beyond 32 767 faces the kernel stages every 32nd table entry instead of every 16th and halves the window once
    out.append(("F40000-N1000", 40000, "plain", 1000))
    return out


def honest_margin(F):
    """A sample nearer to a table boundary than this (as a share of A) could get another face from another summation order"""
    return F * 2.0 ** -50
