"""What the 3-nearest-neighbour kernels of csrc/knn.hip (`distCUDA2`) are checked against, in plain numpy:

1. `mean_dist2_fp64`: the DEFINITION in float64 - mean squared distance to the three nearest neighbours.
2. the fp32 RESTATEMENT of the device code (`box`, `grid_setup`, `grid_plan`, `grid_knn`, `brute`): the box by ordered
   keys, the grid from the box (gridfit_reference.py, pinned to csrc/gridscan.h by test_gridfit_cpu.py), the counting
   sort, the shells of cells and the `reach` stop rule.  tests/test_knn_grid_cpu.py checks it on generic clouds.
3. `CASES`: the boundary table that tests/test_gpu_knn_boundaries.py runs on the device; tests/test_knn_boundaries_cpu.py
   proves on (1) and (2) alone that every case reaches the boundary it is named for.
Importable without a GPU."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridfit_reference as G  # noqa: E402

F = np.float32
FLT_MAX = np.finfo(F).max              # an empty neighbour slot (knn.hip: `big`)
CELL_MAX = 4096                        # HGS_KNN_CELL_MAX: a fuller cell sends the cloud to the brute force
MAX_CELLS = 1 << 22                    # HGS_KNN_MAX_CELLS
SCAN_BLOCK = 1024                      # HGS_SCAN_BLOCK


# ---- 1. the definition, float64 ----------------------------------------------------------------------------------------
def _mean3_fp32(best):
    """((b0 + b1) + b2) / 3 in fp32 on the three smallest distances (ascending): an empty slot (FLT_MAX) makes the sum
    overflow to +inf exactly where the device's does"""
    b = np.sort(best, 1).astype(F)
    with np.errstate(over="ignore"):
        return (((b[:, 0] + b[:, 1]).astype(F) + b[:, 2]).astype(F) / F(3.0)).astype(F)


def _three_nearest_on_a_line(x):
    """The three smallest squared distances of points that differ on ONE axis only (x: that axis, float64).  Exact: the
    squared distance is (x_i - x_j)^2, increasing in |x_i - x_j|, so among the points sorted along the axis the k-th nearest
    of a point on either side is its k-th sorted neighbour on that side; a point more than three ranks away has three points
    of its own side between itself and the query, each at least as near.  Hence the three nearest overall (as distances;
    ties give equal values) are among the ranks -3 .. +3."""
    order = np.argsort(x, kind="stable")
    xs = x[order]
    n = len(xs)
    cand = np.full((n, 6), float(FLT_MAX))
    for k, o in enumerate((1, 2, 3)):
        if n > o:
            d = (xs[o:] - xs[:-o]) ** 2
            cand[:-o, 2 * k] = d                   # the neighbour o ranks up
            cand[o:, 2 * k + 1] = d                # ... and o ranks down
    best = np.empty((n, 3))
    best[order] = np.sort(cand, 1)[:, :3]
    return best


def mean_dist2_fp64(pts32, chunk=256):
    """Mean squared distance of every point to its three nearest neighbours, float64 on the fp32-rounded points.  A point's
    own INDEX is no neighbour, duplicates at distance 0 are; a candidate whose distance is not <= FLT_MAX (NaN or inf: a
    non-finite coordinate on either side) is ignored; slots left empty hold FLT_MAX.  The closing ((b0 + b1) + b2) / 3 is
    fp32.  Brute force in chunks of rows (20k points: a few seconds); a cloud that varies on one axis only takes
    `_three_nearest_on_a_line`."""
    p32 = np.ascontiguousarray(pts32, dtype=F)
    assert p32.ndim == 2 and p32.shape[1] == 3
    p = p32.astype(np.float64)
    P = len(p)
    if P == 0:
        return np.zeros(0, F)
    varying = [a for a in range(3) if not np.all(p[:, a] == p[0, a])]
    if np.isfinite(p).all() and len(varying) == 1:
        return _mean3_fp32(_three_nearest_on_a_line(p[:, varying[0]]))
    best = np.empty((P, 3))
    pad = np.full((min(chunk, P), 3), float(FLT_MAX))
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, P, chunk):
            q = p[i0:i0 + chunk]
            d = (q[:, None, 0] - p[None, :, 0]) ** 2
            d += (q[:, None, 1] - p[None, :, 1]) ** 2
            d += (q[:, None, 2] - p[None, :, 2]) ** 2
            d[~(d <= float(FLT_MAX))] = float(FLT_MAX)
            d[np.arange(len(q)), np.arange(i0, i0 + len(q))] = float(FLT_MAX)
            d = np.concatenate([d, pad[:len(q)]], 1)
            best[i0:i0 + chunk] = np.partition(d, 2, axis=1)[:, :3]
    return _mean3_fp32(best)


# ---- 2. the device code restated, fp32 -----------------------------------------------------------------------------------
def box(pts):
    """hgs_k_knn_bbox: min / max per axis in the order of hgs_float_key (the unsigned image of a float) - on finite values
    the usual order; -NaN sorts below -inf and +NaN above +inf, so a NaN BECOMES the bound it lies beyond."""
    b = np.ascontiguousarray(pts, dtype=F).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))

    def back(k):
        return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F)
    return back(key.min(0)), back(key.max(0))


def grid_plan(pts, nc_max=None):
    """hgs_k_knn_grid_setup + hgs_k_knn_count on a cloud: everything the device decides before it searches.  An axis whose
    extent is not in [0, 3e38) (a NaN or an infinity among its coordinates) collapses to one cell."""
    pts = np.ascontiguousarray(pts, dtype=F)
    P = len(pts)
    nc_max = min(max(64, 2 * P), MAX_CELLS) if nc_max is None else nc_max
    lo, hi = box(pts)
    with np.errstate(invalid="ignore", over="ignore"):
        ext = (hi - lo).astype(F)
        ext = np.where((ext >= 0) & (ext < F(3.0e38)), ext, F(0)).astype(F)
        fitted = P > 8 and ext.max() > 0
        h0 = G.h0_knn(ext, P) if fitted else None
        rounds = G.fit(ext, h0, nc_max)[2] if fitted else 0
        lo, h, inv_h, g = G.grid(lo, ext, h0, nc_max)
        cells = G.cell1(pts, lo, inv_h, g)
    key = (cells[:, 2] * g[1] + cells[:, 1]) * g[0] + cells[:, 0]
    ncells = int(np.prod(g))
    count = np.bincount(key, minlength=ncells) if key.min() >= 0 else None
    Plan = namedtuple("Plan", "lo ext h0 h inv_h g rounds nc_max ncells cells key count")
    return Plan(lo, ext, h0, h, inv_h, g, rounds, nc_max, ncells, cells, key, count)


def grid_setup(pts, nc_max):
    """(lo, h, 1 / h, g) of hgs_k_knn_grid_setup"""
    pl = grid_plan(pts, nc_max)
    return pl.lo, pl.h, pl.inv_h, pl.g


cell_of = G.cell1


def _insert(best, d):
    """the branch-free insert of both kernels; a distance that is not <= FLT_MAX is no candidate"""
    if not d <= FLT_MAX:
        return best
    return sorted(best + [d])[:3]


def grid_knn(pts):
    """hgs_k_knn_search -> (mean squared distances, candidates visited per point, g); None: the device takes the brute force"""
    pts = np.ascontiguousarray(pts, dtype=F)
    P = len(pts)
    pl = grid_plan(pts)
    lo, h, g, cells = pl.lo, pl.h, pl.g, pl.cells
    buckets = {}
    for i, k in enumerate(pl.key):
        buckets.setdefault(int(k), []).append(i)
    if max(len(v) for v in buckets.values()) > CELL_MAX:
        return None
    best3 = np.zeros((P, 3), F)
    visited_total = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(P):
            me, (cx, cy, cz) = pts[i], cells[i]
            best = [FLT_MAX] * 3
            for r in range(0, int(g.max()) + 1):
                z0, z1, y0, y1 = max(cz - r, 0), min(cz + r, g[2] - 1), max(cy - r, 0), min(cy + r, g[1] - 1)
                x0, x1 = max(cx - r, 0), min(cx + r, g[0] - 1)
                for z in range(z0, z1 + 1):
                    for y in range(y0, y1 + 1):
                        if abs(z - cz) == r or abs(y - cy) == r:
                            xs = range(x0, x1 + 1)
                        else:
                            xs = [x for x in (cx - r, cx + r) if 0 <= x <= g[0] - 1]
                            if r == 0:
                                xs = xs[:1]
                        for x in xs:
                            for j in buckets.get(int((z * g[1] + y) * g[0] + x), ()):
                                visited_total += 1
                                if j == i:
                                    continue
                                d = pts[j] - me
                                best = _insert(best, F(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
                if x0 == 0 and y0 == 0 and z0 == 0 and x1 == g[0] - 1 and y1 == g[1] - 1 and z1 == g[2] - 1:
                    break
                reach = FLT_MAX
                for a, c in enumerate((cx, cy, cz)):
                    rel = F(me[a] - lo[a])                      # grid-relative, like the cell assignment (knn.hip)
                    if c - r > 0:
                        reach = min(reach, F(rel - F(F(c - r) * h)))
                    if c + r < g[a] - 1:
                        reach = min(reach, F(F(F(c + r + 1) * h) - rel))
                reach = max(F(reach - F(1e-3) * h), F(0))
                if best[2] <= reach * reach:
                    break
            best3[i] = best
    return _mean3_fp32(best3), visited_total / P, g


def brute(pts):
    """hgs_k_knn3: every pair"""
    p = np.ascontiguousarray(pts, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((p[:, None, :] - p[None, :, :]) ** 2).astype(F)
        d = (d[..., 0] + d[..., 1]).astype(F) + d[..., 2]
    d[~(d <= FLT_MAX)] = FLT_MAX
    np.fill_diagonal(d, FLT_MAX)
    d = np.concatenate([d, np.full((len(p), 3), FLT_MAX, F)], 1)
    return _mean3_fp32(np.sort(d, 1)[:, :3])


# ---- 3. the boundary table -----------------------------------------------------------------------------------------------
# name, builder (-> (P, 3) float32), the boundary it is for; `restate`: small and sparse enough for the Python loops of
# grid_knn; `bad`: indices of the points with a non-finite coordinate
Case = namedtuple("Case", "name build boundary restate bad", defaults=(True, ()))


def _gauss(P, seed=0):
    return lambda: np.random.default_rng(1000 + P + seed).normal(0, 0.4, (P, 3)).astype(F)


def _cluster_in_one_cell(n):
    """n distinct points packed into one cell, and a sparse shell (the corners of [-1, 1]^3 and 96 points near its faces)
    that fixes the box and with it the grid: the cluster's cell is the fullest, with exactly n points"""
    def build():
        rng = np.random.default_rng(7)
        shell = rng.uniform(-1, 1, (96, 3))
        shell[np.arange(96), rng.integers(0, 3, 96)] = rng.choice([-0.9, 0.9], 96)
        corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float)
        cluster = rng.uniform(0.0, 0.03, (4097, 3))[:n]         # (the twin is the same cluster plus one point)
        return np.concatenate([corners, shell, cluster]).astype(F)
    return build


def _box_cloud(ex, P):
    """P uniform points in [0, ex] x [0, 1]^2, two of them on opposite corners"""
    def build():
        pts = np.random.default_rng(11).uniform(0, 1, (P, 3)) * np.array([ex, 1.0, 1.0])
        pts[0], pts[1] = (0, 0, 0), (ex, 1, 1)
        return pts.astype(F)
    return build


def _all_equal(P):
    return lambda: np.full((P, 3), 0.25, F)


def _outliers_in_a_plane():
    """a small dense cluster and four far points that stretch the box to a 100 x 100 slab: the first cell edge asks for
    64 x 64 cells, four times what the scratch was sized for"""
    pts = np.random.default_rng(13).normal(0, 0.01, (504, 3))
    pts[:4] = [(50, 0, 0), (-50, 0, 0), (0, 50, 0), (0, -50, 0)]
    return pts.astype(F)


def _collinear(P):
    def build():
        x = np.random.default_rng(17).uniform(-3, 3, P)
        x[0], x[1] = -3, 3
        return np.stack([x, np.full(P, 0.5), np.full(P, -0.25)], 1).astype(F)
    return build


LATTICE_N, LATTICE_FILL = 12, 1000


def _lattice(shift=0.0):
    """A 12^3 lattice whose spacing IS the cell edge the grid rule yields for the cloud, its first node on the box's low
    corner: every node lies on a cell's face (up to the rounding of the cell assignment itself), and every distance is
    tied many times over.  The box is the cube [-1, 1]^3, fixed by its corners; the first 1000 nodes are there twice
    (distance 0 counts), which brings the cloud to the 2736 points at which twelve cell edges fit into the box."""
    def build():
        n = LATTICE_N
        P = n ** 3 + 8 + LATTICE_FILL
        ext = np.full(3, 2.0, F)
        h = G.fit(ext, G.h0_knn(ext, P), min(max(64, 2 * P), MAX_CELLS))[0]
        i = np.arange(n, dtype=F)
        ax = (F(-1.0) + i * h).astype(F)
        nodes = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
        corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F)
        pts = np.concatenate([corners, nodes, nodes[:LATTICE_FILL]]).astype(F)
        return (pts + F(shift)).astype(F)
    return build


NONFINITE_P = 600
BAD = 123                              # the point that is made non-finite (and BAD + 1 where there are two)


def _nonfinite(edits):
    def build():
        pts = _gauss(NONFINITE_P, seed=5)()
        for i, a, v in edits:
            pts[i, a] = v
        return pts
    return build


NEG_NAN = np.array([0xFFC00000], np.uint32).view(F)[0]
POS_NAN = np.array([0x7FC00000], np.uint32).view(F)[0]
AXIS_P_BELOW, AXIS_P_ABOVE = 137_000, 138_000      # a collinear cloud asks for cbrt(P / 2e-6) cells: 4091 | 4101

CASES = (
    [Case(f"gauss_{P}", _gauss(P), f"P = {P}") for P in (1, 2, 3, 4, 8, 9, 255, 256, 257, 1023, 1024, 1025)]
    + [
        Case("cell_4096", _cluster_in_one_cell(4096), "fullest cell == HGS_KNN_CELL_MAX: the last grid search", restate=False),
        Case("cell_4097", _cluster_in_one_cell(4097), "fullest cell == HGS_KNN_CELL_MAX + 1: the first brute force", restate=False),
        Case("cells_1024", _box_cloud(2.0, 1820), "ncells <= 1024: one scan block"),
        Case("cells_1025", _box_cloud(2.1, 1912), "ncells >= 1025: two scan blocks"),
        Case("all_equal_40", _all_equal(40), "ncells == 1"),
        Case("all_equal_4097", _all_equal(4097), "ncells == 1 and more than HGS_KNN_CELL_MAX points in it", restate=False),
        Case("nc_max_outliers", _outliers_in_a_plane, "the grid is cut down to nc_max cells: hgs_grid_fit grows h"),
        Case("axis_below_limit", _collinear(AXIS_P_BELOW), "the longest axis hgs_grid_fit accepts as asked", restate=False),
        Case("axis_limit", _collinear(AXIS_P_ABOVE), "HGS_GRID_AXIS_MAX alone makes hgs_grid_fit grow h", restate=False),
        Case("lattice", _lattice(), "points on cell faces, massive distance ties"),
        Case("lattice_1e3", _lattice(1.0e3), "the lattice translated by 1e3"),
        Case("nan_pos", _nonfinite([(BAD, 0, POS_NAN)]), "one +NaN coordinate", bad=(BAD,)),
        Case("nan_neg", _nonfinite([(BAD, 1, NEG_NAN)]), "one -NaN coordinate", bad=(BAD,)),
        Case("inf_pos", _nonfinite([(BAD, 2, np.inf)]), "one +inf coordinate", bad=(BAD,)),
        Case("inf_neg", _nonfinite([(BAD, 0, -np.inf)]), "one -inf coordinate", bad=(BAD,)),
        Case("inf_twice", _nonfinite([(BAD, 1, np.inf), (BAD + 1, 1, np.inf)]), "two points at the same +inf", bad=(BAD, BAD + 1)),
        Case("nan_all_axes", _nonfinite([(BAD, 0, POS_NAN), (BAD, 1, POS_NAN), (BAD, 2, POS_NAN)]), "a NaN on every axis of a point",
             bad=(BAD,)),
    ])
BY_NAME = {c.name: c for c in CASES}
RTOL, ATOL = 2e-5, 1e-9


@functools.lru_cache(maxsize=None)
def points(name):
    pts = np.ascontiguousarray(BY_NAME[name].build(), dtype=F)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def expected(name):
    want = mean_dist2_fp64(points(name))
    want.setflags(write=False)
    return want


def mismatch(got, want):
    """None if `got` meets `want` the way the sweep asks - no NaN, +inf exactly where `want` has it, the finite values within
    RTOL / ATOL - or a line that says what does not"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    if np.isnan(got).any():
        return f"{int(np.isnan(got).sum())} NaN, first at {int(np.flatnonzero(np.isnan(got))[0])}"
    inf = np.isinf(want)
    if not np.array_equal(got[inf], want[inf]):
        return f"+inf expected at {np.flatnonzero(inf)[:5]}, got {got[inf][:5]}"
    g, w = got[~inf].astype(np.float64), want[~inf].astype(np.float64)
    bad = ~(np.abs(g - w) <= ATOL + RTOL * np.abs(w))
    if bad.any():
        rel = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
        return f"{int(bad.sum())} of {len(w)} values off, worst relative error {rel[bad].max():.3g} (got {g[bad][0]!r}, want {w[bad][0]!r})"
    return None
