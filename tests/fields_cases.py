"""The case table of the density field's sweep over its launch forms (csrc/fields.hip: hgs_k_field_eval; csrc/api.hip:
hgs_field_eval), shared by tests/test_fields_forms_cpu.py and tests/test_gpu_fields_forms.py.  Pure numpy: imports without a
GPU.

For a split s = resolution / num_blocks a thread owns the samples xp and xp + ceil(s / 2) of one (y, z) column, so a block has
items = ceil(s / 2) s^2 work items; a workgroup has 64 threads when items <= 64 and 256 otherwise, and a block is cut into
slabs = ceil(items / threads) workgroups.  `eval_form` restates that from the constants PARSED out of the two sources
(`constants`): a constant that can no longer be found fails the CPU module.

  A_TABLE   resolution -> block counts.  With relax_ratio = 1.5 * num_blocks (a growth of 3 normalised units) every block
            lists every kept Gaussian, in ascending index: the field is the same bit for bit for every num_blocks.
  B_CASES   cut lists (relax_ratio 1.5, and 0: Gaussians in no block), one case per form and per kind of num_blocks.
  C_FORMS   x c_lengths(): a list of exactly K records, K on both sides of one and of two staging chunks, in both thread forms.
  D_CASES   x D_FORMS: the kept rows of a cloud scattered among dead rows: the compaction strides of hgs_k_field_lists.
  clouds_e  clouds whose kept Gaussians span no extent.
  refused   dimensions that raise before any launch; ACCEPTED: ones the reference's float assertion refused.

Every cloud is seeded and is a kept cloud plus "dead" rows of four kinds (`DEAD_KINDS`): opacity exactly 0.005f, opacity 0,
a NaN coordinate, an infinite coordinate under a high opacity.  The dead rows with finite coordinates lie far outside the
kept cloud, so one that reached the box would move the centre and the scale."""
import functools
import os
import re

import numpy as np

import fields_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "humangaussian_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the forms

def _find(text, pattern, what):
    m = re.search(pattern, text)
    assert m is not None, f"cannot find {what} in the sources any more: the case table of tests/fields_cases.py hangs on it"
    return m


@functools.lru_cache(maxsize=None)
def constants():
    fld = open(os.path.join(CSRC, "fields.hip")).read()
    api = open(os.path.join(CSRC, "api.hip")).read()
    d = lambda name: int(_find(fld, r"#define\s+%s\s+(\d+)u?\b" % name, name).group(1))  # noqa: E731
    c = dict(CHUNK=d("HGS_FIELD_CHUNK"), MAX_BLOCKS=d("HGS_FIELD_MAX_BLOCKS"), MAX_SPLIT=d("HGS_FIELD_MAX_SPLIT"),
             MAX_RES=d("HGS_FIELD_MAX_RES"))
    _find(api, r"const int items = \(\(D\.split \+ 1\) / 2\) \* D\.split \* D\.split;", "the work items of a block")
    m = _find(api, r"const int threads = items <= (\d+) \? (\d+) : (\d+);", "the workgroup size rule")
    c["SMALL_ITEMS"], c["SMALL_THREADS"], c["THREADS"] = (int(v) for v in m.groups())
    _find(api, r"const int slabs = \(items \+ threads - 1\) / threads;", "the slabs of a block")
    _find(fld, r"const int s = D\.split, half = \(s \+ 1\) / 2;", "the two samples of a thread")
    return c


def eval_form(s):
    """(items, threads, slabs, odd) of hgs_k_field_eval's launch for the split s."""
    c = constants()
    items = -(-s // 2) * s * s
    threads = c["SMALL_THREADS"] if items <= c["SMALL_ITEMS"] else c["THREADS"]
    return items, threads, -(-items // threads), s % 2 == 1


ALL_LISTED = 1.5            # relax_ratio = ALL_LISTED * num_blocks grows every block by 3: past the whole cloud (|n| <= 0.9)


def all_listed(nb):
    return ALL_LISTED * nb


# ------------------------------------------------------------------------------------------------ the clouds

DEAD_KINDS = ("opacity == cut", "opacity 0", "nan coordinate", "inf coordinate")


def avatar(n, seed):
    """The recipe of tests/test_gpu_fields.py: points on the humanoid of synth, anisotropic scales, random rotations."""
    from humangaussian_amd import synth
    rng = np.random.default_rng(seed)
    xyz = synth.humanoid_points(n, seed=seed).astype(np.float32)
    scaling = (0.012 * np.exp(0.5 * rng.normal(size=(n, 3)))).astype(np.float32)
    rotation = rng.normal(size=(n, 4)).astype(np.float32)
    opacity = (0.002 + 0.95 * rng.uniform(size=(n, 1))).astype(np.float32)
    return xyz, opacity, scaling, rotation


def wide(n, seed):
    """Wide Gaussians: each one is visible at some sample of even a coarse grid, whatever else is listed."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32)
    scaling = (0.08 * np.exp(0.5 * rng.normal(size=(n, 3)))).astype(np.float32)
    rotation = rng.normal(size=(n, 4)).astype(np.float32)
    opacity = (0.05 + 0.9 * rng.uniform(size=(n, 1))).astype(np.float32)
    return xyz, opacity, scaling, rotation


def kept_rows(cloud, limit=None):
    """The rows the field keeps, in order (at most `limit` of them)."""
    keep = np.nonzero((cloud[1].reshape(-1) > FR.OPACITY_CUT) & np.isfinite(cloud[0]).all(1))[0][:limit]
    return tuple(a[keep] for a in cloud)


def dead(n, seed):
    """n rows the field must ignore, the four kinds in turn.  Finite coordinates lie in [-4, -3] u [3, 4]: outside any kept
    cloud of this table, so a dead row that reached the box would show in the centre and the scale."""
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(3, 4, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))).astype(np.float32)
    scaling = (0.05 * np.exp(0.5 * rng.normal(size=(n, 3)))).astype(np.float32)
    rotation = rng.normal(size=(n, 4)).astype(np.float32)
    opacity = np.full((n, 1), 0.9, np.float32)
    kind = np.arange(n) % 4
    opacity[kind == 0] = FR.OPACITY_CUT                               # not above the cut
    opacity[kind == 1] = 0.0
    col = np.arange(n) // 4 % 3
    xyz[kind == 2, col[kind == 2]] = np.nan
    sel = np.nonzero(kind == 3)[0]
    xyz[sel, col[sel]] = np.where(sel // 12 % 2 == 0, np.inf, -np.inf).astype(np.float32)
    return xyz, opacity, scaling, rotation


def scatter(kept, P, seed, pinned=()):
    """The rows of `kept`, in order, at sorted positions of a cloud of P rows - `pinned` first, the others drawn - and dead
    rows everywhere else.  (cloud, positions)."""
    K = len(kept[0])
    pinned = sorted(set(int(i) for i in pinned))
    assert K <= P and len(pinned) <= K and all(0 <= i < P for i in pinned)
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(P), pinned)
    pos = np.sort(np.concatenate([pinned, rng.choice(rest, K - len(pinned), replace=False)]).astype(np.int64))
    out = tuple(a.copy() for a in dead(P, seed + 1))
    for o, k in zip(out, kept):
        o[pos] = k
    return out, pos


# ------------------------------------------------------------------------------------------------ (a) every split

A_TABLE = {24: (1, 2, 3, 4, 6, 8, 12, 24), 40: (1, 2, 4, 5, 8, 10, 20), 56: (1, 2, 4, 7, 8, 14, 28),
           72: (2, 3, 4, 6, 8, 9, 12, 18, 24)}
A_PINNED_SPLIT = 8          # the form the existing suite already holds to fp64; every resolution of A_TABLE contains it
A_GATED_RES = 72            # ... and here the pinned split passes the fp64 gate once more, on this cloud


@functools.lru_cache(maxsize=None)
def cloud_a():
    """About 400 rows (more than one staging chunk): 380 of the avatar recipe and 24 dead ones among them."""
    kept = kept_rows(avatar(380, 21))
    return scatter(kept, len(kept[0]) + 24, 22)[0]


# ------------------------------------------------------------------------------------------------ (b) cut lists

# (resolution, num_blocks, relax_ratio, rows, seed).  The seeds were chosen so that the restatement alone flags at most
# 0.1 % of the blocks as "a Gaussian within 1e-6 of a cut plane" (tests/test_fields_forms_cpu.py holds them to it).
B_CASES = [
    (72, 9, 1.5, 3000, 32),      # s = 8, nb not a power of two
    (72, 8, 1.5, 3000, 32),      # s = 9: odd, two slabs
    (56, 8, 1.5, 3000, 32),      # s = 7
    (60, 12, 1.5, 3000, 32),     # s = 5
    (66, 22, 1.5, 3000, 32),     # s = 3
    (64, 32, 1.5, 3000, 32),     # s = 2, the largest nb
    (32, 32, 1.5, 3000, 32),     # s = 1
    (64, 4, 1.5, 1500, 32),      # s = 16, eight slabs
    (48, 3, 1.5, 1500, 32),      # s = 16, nb = 3
    (40, 1, 1.5, 1500, 32),      # one block (s = 40, 125 slabs)
    (72, 8, 0.0, 3000, 32),      # Gaussians between two blocks' sample ranges are in no block
    (60, 12, 0.0, 3000, 32),
    (32, 32, 0.0, 3000, 32),     # a block is one point and the test is strict: nothing is listed at all
]
B_DEAD = 40
FLAGGED_CAP = 1e-3


def b_id(case):
    return "R%d-nb%d-relax%g" % case[:3]


@functools.lru_cache(maxsize=None)
def cloud_b(rows, seed):
    kept = kept_rows(avatar(rows - B_DEAD, seed))
    return scatter(kept, len(kept[0]) + B_DEAD, seed + 100)[0]


# ------------------------------------------------------------------------------------------------ (c) list lengths

C_FORMS = [(8, 2), (20, 2)]          # s = 4: 64 threads stage 256 records;  s = 10: 256 threads, two slabs
C_DEAD = 9
PRESENCE = 1e-2                      # every record carries at least this share of the fp64 field at some sample


def c_lengths():
    c = constants()["CHUNK"]
    return [2, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1]


@functools.lru_cache(maxsize=None)
def cloud_c(K):
    """K wide Gaussians, every one visible in both forms, and C_DEAD dead rows among them.  The plain recipe does not give
    that on the 8^3 grid (samples 0.29 apart): of 513 draws a few dozen are narrow and sit between the samples, where
    they carry 1e-3 .. 1e-4 of the field and could be lost under the gate.  Those rows are drawn again, from the same
    recipe, until every row carries twice PRESENCE somewhere (the CPU module then holds the cloud to PRESENCE itself)."""
    cloud = tuple(a.copy() for a in wide(K, 500 + K))
    for again in range(1, 40):
        weak = np.zeros(K, bool)
        for R, nb in C_FORMS:
            weak |= presence(cloud, R, nb) < 2 * PRESENCE
        if not weak.any():
            break
        for a, b in zip(cloud, wide(K, 500 + K + 1000 * again)):
            a[weak] = b[weak]
    assert not weak.any(), (K, int(weak.sum()))
    return scatter(cloud, K + C_DEAD, 700 + K)[0]


def presence(cloud, resolution, num_blocks):
    """Per kept Gaussian: its largest share of the fp64 field over the samples (all-listed: one list for every block)."""
    P = FR.prepare(*cloud, resolution, num_blocks, all_listed(num_blocks), np.float64)
    co = FR.inverse_coefficients(P, np.float64)
    ax = P.axis.astype(np.float64)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 1, 3) - P.n[None]
    x, y, z = g[..., 0], g[..., 1], g[..., 2]
    power = (-0.5 * (x * x * co[:, 0] + y * y * co[:, 3] + z * z * co[:, 5]) - x * y * co[:, 1] - x * z * co[:, 2]
             - y * z * co[:, 4])
    w = P.opacity * np.where(power > 0, 0.0, np.exp(np.minimum(power, 0.0)))
    total = w.sum(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0, w / total, 0.0).max(0)


# ------------------------------------------------------------------------------------------------ (d) dead rows

# (rows P, kept rows K): P = 1025 takes the K ~ 300 cloud, P = 257 cannot hold 300 kept rows beside dead ones and takes the
# first 150 of them.  Kept rows sit on both sides of the 64-lane ballot and of the 256-row stride of hgs_k_field_lists.
D_CASES = [(1025, 300), (257, 150)]
D_FORMS = [(32, 8, 1.5), (20, 2, all_listed(2))]      # cut lists; all-listed


def d_pinned(P):
    return [i for i in (0, 63, 64, 255, 256, 257, P - 1) if i < P]


@functools.lru_cache(maxsize=None)
def cloud_d(P, K):
    """(scattered cloud of P rows, the same kept rows compacted, their positions)."""
    kept = kept_rows(avatar(320, 41), K)
    assert len(kept[0]) == K
    scattered, pos = scatter(kept, P, 42 + P, d_pinned(P))
    return scattered, kept, pos


# ------------------------------------------------------------------------------------------------ (e) no extent

def clouds_e():
    """name -> (cloud, the point).  The reference divides by zero here: the contract is "no NaN, nothing listed"."""
    one = tuple(a[:1] for a in wide(1, 61))
    among, pos = scatter(tuple(a[:1] for a in wide(1, 62)), 70, 63, pinned=[37])
    five = wide(5, 64)
    five[0][:] = five[0][2].copy()
    return {"one row": (one, one[0][0]), "one kept row among dead ones": (among, among[0][pos[0]]),
            "five coincident rows": (five, five[0][0])}


# ------------------------------------------------------------------------------------------------ (f) refused

def refused():
    """(resolution, num_blocks) that raise before any launch, from the parsed limits."""
    c = constants()
    return [(32, 0), (c["MAX_BLOCKS"] + 1, c["MAX_BLOCKS"] + 1), (c["MAX_RES"] + 1, 1),
            ((c["MAX_SPLIT"] + 1) * 2, 2), (100, 16), (33, 2)]


ACCEPTED = [(30, 3), (63, 9), (36, 9)]      # resolution % (2 / num_blocks) != 0 in floating point, and perfectly good


# ------------------------------------------------------------------------------------------------ the fp64 gate

REL_FLOOR = 1e-4     # twice the largest kernel distance profiles/fields_parity.json records (4.99e-5): on the coarse grids
                     # of this sweep e is a maximum over few samples and falls to the kernel's own fp32 rounding


def gate_bounds(e, field_max):
    """(relative bound over the samples above 1e-3 of the maximum, absolute bound below) for e = distance(fp32 formula, fp64)."""
    b = max(1.25 * e, REL_FLOOR)
    return b, b * 1e-3 * field_max


def kernel_distance(occ, ref64, clean=None):
    """(relative, absolute) distance of tests/test_gpu_fields.py over the samples of `clean`."""
    clean = np.ones(ref64.shape, bool) if clean is None else clean
    o = np.asarray(occ, np.float64)
    big = (ref64 > 1e-3 * ref64.max()) & clean
    small = ~(ref64 > 1e-3 * ref64.max()) & clean
    rel = float((np.abs(o - ref64)[big] / ref64[big]).max()) if big.any() else 0.0
    ab = float(np.abs(o - ref64)[small].max()) if small.any() else 0.0
    return rel, ab


@functools.lru_cache(maxsize=None)
def _reference(key):
    cloud, R, nb, relax = _REF_ARGS[key]
    ref64, P = FR.field(*cloud, resolution=R, num_blocks=nb, relax_ratio=relax, dtype=np.float64)
    ref32, _ = FR.field(*cloud, resolution=R, num_blocks=nb, relax_ratio=relax, dtype=np.float32)
    for a in (ref64, ref32):
        a.setflags(write=False)
    return ref64, ref32, P


_REF_ARGS = {}


def reference(key, cloud, R, nb, relax):
    """(fp64 field, the reference's formula in fp32, Prepared) of a case, computed once per process and read-only."""
    _REF_ARGS[key] = (cloud, R, nb, relax)
    return _reference(key)
