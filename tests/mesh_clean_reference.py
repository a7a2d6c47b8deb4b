"""numpy restatement of include/hgs_rast.h's mesh cleaning and decimation (hgs_meshclean_*), written from the header's
definitions: components by breadth-first search and by an emulation of the label rounds, the keep rule, the bisection
over the clustering grid, the integer-lattice means and the duplicate rule.  No GPU, no torch.  Every fp32 operation
of the header is one numpy float32 operation here, so the results are comparable bit for bit."""
import numpy as np

f32 = np.float32
G_MAX = 1024
LATTICE = 1048576


def _f(vertices):
    return np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)


def _i(faces):
    return np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)


def valid_faces(V, faces):
    """mask of the faces whose three indices lie in [0, V)"""
    faces = _i(faces)
    return ((faces >= 0) & (faces < V)).all(axis=1)


def box(vertices):
    """(lo (3,), ext (3,), emax) in fp32 of the finite vertices; None without one"""
    v = _f(vertices)
    v = v[np.isfinite(v).all(axis=1)]
    if v.shape[0] == 0:
        return None
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = (hi - lo).astype(f32)
    return lo, ext, f32(ext.max())


def diag2(vertices):
    """(dx dx + dy dy) + dz dz in fp32 of the box of the finite vertices; 0 without one"""
    b = box(vertices)
    if b is None:
        return f32(0)
    e = b[1]
    with np.errstate(over="ignore"):
        return f32(f32(f32(e[0] * e[0]) + f32(e[1] * e[1])) + f32(e[2] * e[2]))


# ---- components --------------------------------------------------------------------------------------------------------
def components_bfs(V, faces):
    """labels[v] = the smallest vertex index of v's component"""
    faces = _i(faces)
    faces = faces[valid_faces(V, faces)]
    src = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2], faces[:, 1], faces[:, 2], faces[:, 0]])
    dst = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0], faces[:, 0], faces[:, 1], faces[:, 2]])
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    start = np.searchsorted(src, np.arange(V + 1))
    labels = np.full(V, -1, dtype=np.int64)
    for s in range(V):                       # ascending: the first vertex that reaches a component is its smallest
        if labels[s] >= 0:
            continue
        labels[s] = s
        frontier = np.array([s])
        while frontier.size:
            nb = np.concatenate([dst[start[u]:start[u + 1]] for u in frontier]) if frontier.size else frontier
            nb = np.unique(nb)
            nb = nb[labels[nb] < 0]
            labels[nb] = s
            frontier = nb
    return labels.astype(np.int32)


def components_rounds(V, faces, hook_roots=True):
    """(labels, rounds): the header's rounds, every round reading the labels the round before left - per face the
    minimum of its three labels into the three labels and (hook_roots) into the labels' own labels, then one
    pointer-jumping pass.  `rounds` counts the last round too, the one that changed nothing."""
    faces = _i(faces)
    faces = faces[valid_faces(V, faces)]
    labels = np.arange(V, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        old = labels
        lab = old[faces]
        m = lab.min(axis=1) if faces.shape[0] else np.zeros(0, dtype=np.int64)
        new = old.copy()
        for k in range(3):
            np.minimum.at(new, faces[:, k], m)
            if hook_roots:
                np.minimum.at(new, lab[:, k], m)
        labels = new[new]
        if np.array_equal(labels, old):
            return labels.astype(np.int32), rounds


def component_stats(vertices, faces, labels):
    """(comp_faces (V,) int32, comp_diag2 (V,) fp32): per component at its label, 0 elsewhere"""
    v, faces = _f(vertices), _i(faces)
    V = v.shape[0]
    faces = faces[valid_faces(V, faces)]
    comp_faces = np.zeros(V, dtype=np.int32)
    np.add.at(comp_faces, labels[faces[:, 0]], 1)
    comp_diag2 = np.zeros(V, dtype=np.float32)
    order = np.argsort(labels, kind="stable")
    bounds = np.flatnonzero(np.diff(labels[order], prepend=-1))
    for lo, hi in zip(bounds, list(bounds[1:]) + [V]):
        comp_diag2[labels[order[lo]]] = diag2(v[order[lo:hi]])
    return comp_faces, comp_diag2


# ---- clean ---------------------------------------------------------------------------------------------------------------
def keep_threshold(vertices, min_d):
    p = f32(f32(min_d) / f32(100.0))
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(f32(p * p) * diag2(vertices))


def clean(vertices, faces, min_f=64, min_d=20.0, labels=None):
    """(vertices', faces' int32, vertex_src int32)"""
    v, faces = _f(vertices), _i(faces)
    V = v.shape[0]
    if labels is None:
        labels = components_bfs(V, faces)
    comp_faces, comp_diag2 = component_stats(v, faces, labels)
    ok = valid_faces(V, faces)
    fs = np.where(ok[:, None], faces, 0)
    distinct = (fs[:, 0] != fs[:, 1]) & (fs[:, 1] != fs[:, 2]) & (fs[:, 0] != fs[:, 2])
    L = labels[fs[:, 0]]
    keep = ok & distinct & (comp_faces[L] >= min_f) & ~(comp_diag2[L] < keep_threshold(v, min_d))
    vkeep = np.zeros(V, dtype=bool)
    vkeep[faces[keep].reshape(-1)] = True
    vertex_src = np.flatnonzero(vkeep)
    new_of_old = np.full(V, -1, dtype=np.int64)
    new_of_old[vertex_src] = np.arange(vertex_src.size)
    return v[vertex_src], new_of_old[faces[keep]].astype(np.int32).reshape(-1, 3), vertex_src.astype(np.int32)


# ---- decimate ------------------------------------------------------------------------------------------------------------
def _box_or_nan(vertices):
    b = box(vertices)
    if b is None:
        nan = f32(np.nan)
        return np.full(3, nan, dtype=np.float32), np.full(3, nan, dtype=np.float32), nan
    return b


def cell_keys(vertices, g):
    """30-bit cell key of every vertex on the grid of g cells per axis: hgs_grid_cell1 per axis"""
    v = _f(vertices)
    lo, _, emax = _box_or_nan(v)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv_h = f32(f32(g) / emax)
        t = np.floor(((v - lo).astype(f32) * inv_h).astype(f32))
        c = np.fmin(np.fmax(t, f32(0)), f32(g - 1)).astype(np.int64)
    return (c[:, 2] * g + c[:, 1]) * g + c[:, 0]


def surviving(vertices, faces, g):
    v, faces = _f(vertices), _i(faces)
    faces = faces[valid_faces(v.shape[0], faces)]
    k = cell_keys(v, g)[faces]
    return int(((k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])).sum())


def choose_grid(vertices, faces, target):
    """(g, probes): the header's bisection and nothing else"""
    lo, hi, probes = 1, G_MAX + 1, 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probes += 1
        if surviving(vertices, faces, mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo, probes


def lattice(vertices):
    """(q (V,3) int64, lo (3,) fp32, emax fp32)"""
    v = _f(vertices)
    lo, _, emax = _box_or_nan(v)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        qs = f32(f32(LATTICE) / emax)
        t = np.floor((((v - lo).astype(f32) * qs).astype(f32) + f32(0.5)).astype(f32))
        q = np.fmin(np.fmax(t, f32(0)), f32(LATTICE)).astype(np.int64)
    return q, lo, emax


def cluster(vertices, faces, g):
    """(vertices', faces' int32, rep (V,)) of the clustering on the grid of g cells per axis"""
    v, faces = _f(vertices), _i(faces)
    V = v.shape[0]
    keys = cell_keys(v, g)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    rep = first[inverse.reshape(-1)]                           # the smallest vertex index of the vertex's cell
    ok = valid_faces(V, faces)
    r = rep[np.where(ok[:, None], faces, 0)]
    surv = np.flatnonzero(ok & (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2]))
    if surv.size:
        _, firsts = np.unique(np.sort(r[surv], axis=1), axis=0, return_index=True)
        kept = surv[np.sort(firsts)]                         # of each vertex set the lowest original index
    else:
        kept = surv
    used = np.unique(r[kept].reshape(-1))                     # ascending representative = ascending smallest member
    q, lo, emax = lattice(v)
    sums = np.zeros((V, 3), dtype=np.int64)
    np.add.at(sums, rep, q)
    cnt = np.bincount(rep, minlength=V)
    with np.errstate(invalid="ignore", over="ignore"):
        m = sums[used].astype(np.float64) / cnt[used].astype(np.float64)[:, None]
        pos = (lo.astype(np.float64)[None, :] + m * (np.float64(emax) / np.float64(LATTICE))).astype(np.float32)
    new_of_old = np.full(V, -1, dtype=np.int64)
    new_of_old[used] = np.arange(used.size)
    return pos.reshape(-1, 3), new_of_old[r[kept]].astype(np.int32).reshape(-1, 3), rep


def decimate(vertices, faces, target):
    """(vertices', faces' int32, info): info = None for the no-op cases, else {"grid", "cell", "input_faces"}"""
    v, faces = _f(vertices), _i(faces)
    F = faces.shape[0]
    if target <= 0 or F <= target:
        return v, faces.astype(np.int32), None
    g, probes = choose_grid(v, faces, target)
    nv, nf, _ = cluster(v, faces, g)
    emax = _box_or_nan(v)[2]
    return nv, nf, {"grid": g, "cell": float(f32(emax / f32(g))), "input_faces": F, "probes": probes}


# ---- test meshes (shared by test_mesh_clean_cpu.py and test_gpu_mesh_clean.py) ----------------------------------------------
TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int64)
TET_XYZ = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)


def permute_vertices(vertices, faces, perm):
    """the same mesh with old vertex i stored at index perm[i]"""
    v = np.empty_like(vertices)
    v[perm] = vertices
    return v, perm[faces]


def two_tets(interleaved=False):
    """two disjoint tetrahedra and an isolated vertex: 9 vertices, 8 faces"""
    v = np.concatenate([TET_XYZ, TET_XYZ * f32(0.5) + f32(4.0), np.array([[9, 9, 9]], dtype=np.float32)])
    f = np.concatenate([TET, TET + 4])
    if interleaved:
        v, f = permute_vertices(v, f, np.array([0, 2, 4, 6, 1, 3, 5, 7, 8]))
    return v, f


def strip(n=2050, order="natural", seed=0):
    """a triangle strip of n vertices (n - 2 faces): long label chains"""
    i = np.arange(n)
    v = np.stack([(i // 2).astype(np.float32), (i % 2).astype(np.float32), np.zeros(n, dtype=np.float32)], axis=1)
    k = np.arange(n - 2)
    f = np.where((k % 2 == 0)[:, None], np.stack([k, k + 1, k + 2], 1), np.stack([k + 1, k, k + 2], 1))
    perm = {"natural": i, "reversed": i[::-1].copy(), "random": np.random.default_rng(seed).permutation(n)}[order]
    return permute_vertices(v, f, perm)


def torus(nu=40, nv=24, R=2.0, r=0.7):
    u, w = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = 2 * np.pi * u / nu, 2 * np.pi * w / nv
    v = np.stack([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)], -1).reshape(-1, 3)
    idx = lambda p, q: (p % nu) * nv + (q % nv)  # noqa: E731
    f = np.concatenate([np.stack([idx(u, w), idx(u + 1, w), idx(u + 1, w + 1)], -1).reshape(-1, 3),
                        np.stack([idx(u, w), idx(u + 1, w + 1), idx(u, w + 1)], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int64)


def fan_with_floaters(n_rim, seed=0):
    """a closed fan of n_rim + 1 vertices and n_rim + 1 faces (one chord triangle added), three tetrahedra far away and
    five unreferenced vertices, all in seeded-random vertex order: with min_f = 8 exactly n_rim + 1 vertices and faces stay"""
    a = 2 * np.pi * np.arange(n_rim) / n_rim
    v = np.concatenate([np.zeros((1, 3)), np.stack([np.cos(a), np.sin(a), 0 * a], 1)])
    k = np.arange(n_rim)
    f = np.concatenate([np.stack([np.zeros(n_rim, dtype=np.int64), 1 + k, 1 + (k + 1) % n_rim], 1), [[1, 3, 5]]])
    for t in range(3):
        f = np.concatenate([f, TET + v.shape[0]])
        v = np.concatenate([v, TET_XYZ * 0.05 + 3.0 + t])
    v = np.concatenate([v, np.random.default_rng(seed).uniform(-1, 1, (5, 3))])
    perm = np.random.default_rng(seed + 1).permutation(v.shape[0])
    return permute_vertices(v.astype(np.float32), f.astype(np.int64), perm)


def random_soup(nv=5000, nf=9000, seed=0):
    """seeded-random vertices with random faces: nearly every vertex in a cell of its own at a fine grid"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (nv, 3)).astype(np.float32), rng.integers(0, nv, (nf, 3)).astype(np.int64)


def plane_grid(n=8):
    """(n + 1)^2 vertices on the integer lattice of a plane, 2 n^2 faces: with g = 2, 4, 8 vertices lie exactly on cell planes"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i, j, 0 * i], -1).reshape(-1, 3).astype(np.float32)
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + 1], 1)])
    return v, f.astype(np.int64)


def flipped_pair():
    """Four clusters of three vertices 2^-6 apart at the corners of an 8-box.  Faces 0 and 1 join the clusters A, B, C with
    opposite orientation, faces 2 and 3 go to D; ten small faces inside cluster A come alive only at the finest grids.
    With target = 5 the bisection ends at a grid that collapses every cluster: faces 0 and 1 become duplicates."""
    e = f32(2.0 ** -6)
    corner = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0], [0, 0, 8]], dtype=np.float32)
    sign = np.array([[1, 1, 1], [-1, 1, 1], [1, -1, 1], [1, 1, -1]], dtype=np.float32)
    first = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)          # cluster A: three distinct cells at g = 1024
    other = np.array([[0, 0, 0], [1, 1, 0], [0, 1, 1]], dtype=np.float32)
    v = np.concatenate([corner[c] + sign[c] * e * (first if c == 0 else other) for c in range(4)]).astype(np.float32)
    A, B, C, D = 0, 3, 6, 9
    f = [[A, B, C], [C + 1, B + 1, A + 1], [A + 2, B + 2, D], [A, B + 1, D + 1]] + [[A, A + 1, A + 2]] * 10
    return v, np.array(f, dtype=np.int64)
