"""Scenes whose tile-list and cell-list lengths are PRESCRIBED, not sampled, and the thresholds of the list pipeline
parsed out of the sources (tests/test_gpu_list_boundaries.py builds its cases from them; tests/test_list_boundaries_cpu.py
checks the scenes on the oracle alone).

A scene is a dict {(tile_x, tile_y, cell): count} seen by the camera of `make_scene(..., elev=0, azim=0)`: jittered pixel
positions around the cell's centre at random depths in [1.5, 2.5], unprojected through the inverse of
`cam.world_view_transform`; scales = sigma_px * z / focal; the Gaussian order shuffled.  Two kinds of Gaussian:

  dot      cell = 0..15.  sigma 0.25 px (the 0.3 px^2 dilation dominates: covariance ~0.36 px^2), jitter +-0.5 px: the
           alpha >= 1/255 ellipse (radius <= 1.9 px at opacity 0.2, <= 1.7 px at 0.13, margins of csrc/cellmask.h included)
           stays between the pixel centres of ONE cell (they span 3 px around the cell's centre: 0.5 + 1.9 < 2.5, 0.75 +
           1.7 < 2.5), and a pixel centre
           is never farther than 0.71 px: every dot is one entry of one tile list and ONE (entry, cell) pair.
  blanket  cell = BLANKET.  sigma 6 px, centred in the tile: all 16 cells, 16 pairs per entry (HGS_PAIRS_PER_ENTRY).

A spec names its dots' opacity range and jitter and the REGIME it claims (tests/test_list_boundaries_cpu.py holds it to the
claim on the oracle): "thin" - no pixel terminates, final T >= 0.05 everywhere, every entry carries gradient (blankets:
0.008 .. 0.011); "thick" - in every cell of at least THICK_MIN dots most of the 16 pixels terminate inside the list, at
cell-list positions in three or more 128-entry segments (jitter 0.75 px puts load on the outer twelve pixels; a cell needs
the dots for it: terminating 9 pixels takes a summed alpha of ~83, a confined dot brings <= 0.3, most of it to the four
central pixels - with 1024 dots only those four terminate); "plain" - claims neither
(mid-length lists, ties: some pixels terminate).  Options: `ties` = k copies of one
position at depth exactly 2.0 with the other depths kept out of (1.99, 2.01), so that the k equal keys have a bucket of the
rank sort to themselves (ties are broken by Gaussian index, like upstream's stable sort); `outlier`: one dot at depth 600
that stretches the depth range, so that the body of the list shares a few buckets."""
import collections
import math
import os
import re

import numpy as np
import torch

import oracle
from helpers import make_scene, oracle_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "humangaussian_amd", "csrc")
BLANKET = -1
DOT_SIGMA, BLANKET_SIGMA = 0.25, 6.0
THICK_MIN = 4096                                # dots in a cell from which a "thick" scene must terminate most of its pixels
BLANKET_OPACITY = (0.008, 0.011)
TIE_DEPTH, TIE_GAP, OUTLIER_DEPTH = 2.0, 0.01, 600.0

Spec = collections.namedtuple("Spec", "name H W counts regime op jitter ties outlier seed")


def spec(name, counts, H=16, W=16, regime="thin", op=(0.01, 0.025), jitter=0.5, ties=0, outlier=False, seed=0):
    assert regime in ("thin", "thick", "plain")
    return Spec(name, H, W, tuple(sorted(counts.items())), regime, tuple(op), jitter, ties, outlier, seed)


def spread(n, cells=range(16), tile=(0, 0)):
    """n dots spread evenly over the cells of one tile"""
    cells = list(cells)
    return {(tile[0], tile[1], c): n // len(cells) + (1 if i < n % len(cells) else 0) for i, c in enumerate(cells)
            if n // len(cells) + (1 if i < n % len(cells) else 0) > 0}


def build(sp):
    """-> the usual scene dict (+ "kind": 0 dot / 1 blanket, "cell", "tile" per Gaussian, after the shuffle)"""
    g = torch.Generator().manual_seed(1000003 * sp.seed + sum(n for _, n in sp.counts) + 7)
    sc = make_scene(P=1, seed=0, H=sp.H, W=sp.W, elev=0.0, azim=0.0, dist=2.0, fovy=50.0)
    cam = sc["cam"]
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    px, py, kind, cell, tile = [], [], [], [], []
    for (tX, tY, c), n in sp.counts:
        if c == BLANKET:
            cx, cy, jit = tX * 16 + 7.5, tY * 16 + 7.5, 0.5
        else:
            cx, cy, jit = tX * 16 + (c % 4) * 4 + 1.5, tY * 16 + (c // 4) * 4 + 1.5, sp.jitter
        px.append(cx + (torch.rand(n, generator=g) - 0.5) * 2 * jit)
        py.append(cy + (torch.rand(n, generator=g) - 0.5) * 2 * jit)
        kind.append(torch.full((n,), 1 if c == BLANKET else 0))
        cell.append(torch.full((n,), c))
        tile.append(torch.full((n,), tY * ((sp.W + 15) // 16) + tX))
    px, py, kind, cell, tile = (torch.cat(v) for v in (px, py, kind, cell, tile))
    P = px.numel()
    perm = torch.randperm(P, generator=g)
    px, py, kind, cell, tile = px[perm], py[perm], kind[perm], cell[perm], tile[perm]
    z = 1.5 + torch.rand(P, generator=g)
    z = torch.where(kind == 1, 2.6 + 0.4 * torch.rand(P, generator=g), z)          # blankets lie under the dots
    if sp.ties:
        near = (z - TIE_DEPTH).abs() < TIE_GAP
        z = torch.where(near, z + torch.where(z < TIE_DEPTH, -TIE_GAP, TIE_GAP), z)
        idx = torch.nonzero(kind == 0).reshape(-1)
        idx = idx[torch.randperm(idx.numel(), generator=g)[: sp.ties]]            # the copies: dots anywhere in the order
        first = int(idx[0])
        px[idx], py[idx], cell[idx], tile[idx] = float(px[first]), float(py[first]), int(cell[first]), int(tile[first])
        z[idx] = TIE_DEPTH
    if sp.outlier:
        z[int(torch.nonzero(kind == 0)[-1])] = OUTLIER_DEPTH
    ndx, ndy = (2 * px + 1) / sp.W - 1, (2 * py + 1) / sp.H - 1
    pc = torch.stack([ndx * tx * z, ndy * ty * z, z, torch.ones(P)], 1).double()
    world = (pc @ torch.linalg.inv(cam.world_view_transform.double())).float()
    if sp.ties:
        world[idx] = world[first].clone()                                                  # bit-equal positions: bit-equal depths
    sc["means3D"] = world[:, :3].contiguous()
    focal = sp.W / (2 * tx)
    sigma = torch.where(kind == 1, torch.tensor(BLANKET_SIGMA), torch.tensor(DOT_SIGMA))
    noise = torch.where(kind == 1, torch.tensor(0.02), torch.tensor(0.1))[:, None] * torch.randn(P, 3, generator=g)
    sc["scales"] = (sigma * z / focal)[:, None] * torch.exp(noise)
    sc["rotations"] = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1)
    lo, hi = sp.op
    u = torch.rand(P, 1, generator=g)
    sc["opacities"] = torch.where(kind[:, None] == 1, BLANKET_OPACITY[0] + (BLANKET_OPACITY[1] - BLANKET_OPACITY[0]) * u,
                                  lo + (hi - lo) * u)
    sc["shs"] = torch.randn(P, 1, 3, generator=g) * 0.8
    sc.update(kind=kind, cell=cell, tile=tile, target=torch.stack([px, py], 1))
    return sc


_SCENES, _REFS = {}, {}


def scene(sp):
    if sp not in _SCENES:
        _SCENES[sp] = build(sp)
    return _SCENES[sp]


def upstream(sp, view=0):
    g = torch.Generator().manual_seed(77 + view)
    return [torch.randn(s, generator=g) for s in ((3, sp.H, sp.W), (1, sp.H, sp.W), (1, sp.H, sp.W))]


def reference(sp, view=0):
    """(fp32 oracle, fp64 oracle) forward + backward of the scene under the incoming gradients of `view`; computed once,
    shared by every test that needs it and never modified"""
    if (sp, view) not in _REFS:
        sc = scene(sp)
        args = (sc["means3D"], sc["shs"], None, sc["opacities"], sc["scales"], sc["rotations"], None, oracle_settings(sc))
        with torch.enable_grad():
            _REFS[(sp, view)] = tuple(oracle.forward_backward(*args, *upstream(sp, view), dtype=dt, want_means2D=True)
                                      for dt in (torch.float32, torch.float64))
    return _REFS[(sp, view)]


def prescribed_lists(sp):
    """{tile index: list length} of the spec"""
    gx = (sp.W + 15) // 16
    out = collections.Counter()
    for (tX, tY, _), n in sp.counts:
        out[tY * gx + tX] += n
    return dict(out)


def prescribed_pairs(sp):
    return sum(n * (16 if c == BLANKET else 1) for (_, _, c), n in sp.counts)


# ------------------------------------------------------------------------------------------------- thresholds of the sources
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(text, pattern, what):
    m = re.search(pattern, text)
    assert m, f"threshold not found in the sources any more: {what} ({pattern})"
    return m


def thresholds():
    """Every switch of the list pipeline named in the docstring of tests/test_gpu_list_boundaries.py, parsed by regular
    expression; a threshold that can no longer be found fails here."""
    com, ent, binn, fwd, api = (_src(n) for n in ("hgs_common.h", "entryrec.h", "binning.hip", "render_fwd.hip", "api.hip"))
    d = lambda text, name: int(_find(text, r"#define\s+%s\s+(\d+)u?\b" % name, name).group(1))  # noqa: E731
    t = dict(RB=d(com, "HGS_RB"), SEGLEN=d(com, "HGS_SEGLEN"), SORT_LDS_MAX=d(com, "HGS_SORT_LDS_MAX"), NFC=d(com, "HGS_NFC"),
             CHUNK_RECS=d(ent, "HGS_CHUNK_RECS"), PAIRS_PER_ENTRY=d(ent, "HGS_PAIRS_PER_ENTRY"),
             BUCKET_MAX=d(binn, "HGS_RANK_BUCKET_MAX"), NB_MAX=d(binn, "HGS_RANK_NB_MAX"), NT=d(binn, "HGS_SORT_NT"),
             GU=d(binn, "HGS_RANK_GU"), FWD_C4=d(fwd, "HGS_FWD_C4"))
    t["NB_MIN"] = int(_find(binn, r"uint32_t NB = (\d+)u;", "the first NB").group(1))
    t["NB_FACTOR"] = int(_find(binn, r"while \(NB < (\d+)u \* n && NB < \(uint32_t\)HGS_RANK_NB_MAX\) NB <<= 1;", "NB doubling").group(1))
    t["KEYS_PER_THREAD"] = [int(_find(binn, r"n <= (\d+)u \* NT\) degenerate = rank_keys<%d, NT>" % e, f"rank_keys<{e}>").group(1))
                            for e in (2, 4)]
    t["EARLY"] = int(_find(binn, r"const bool early = n <= (\d+)u \* NT;", "register form / stream form").group(1))
    _find(binn, r"n <= \(uint32_t\)HGS_SORT_LDS_MAX \|\| n > (\d+)u\) return;", "hgs_k_sort_large's range")
    t["HUGE"] = int(_find(binn, r"if \(n <= (\d+)u\) return;\s*\n\s*__shared__ GatherLds<256> S;\s*\n\s*bitonic_sort<1024>", "hgs_k_sort_huge's range").group(1))
    assert int(_find(api, r"need_huge = hint <= 0 \|\| hint > (\d+)", "need_huge").group(1)) == t["HUGE"]
    _find(api, r"need_large = hint <= 0 \|\| hint > HGS_SORT_LDS_MAX;", "need_large")
    m = _find(api, r"expect_long = hint <= 0 \|\| hint > HGS_SORT_LDS_MAX \+ HGS_SORT_LDS_MAX / (\d+) \+ (\d+);", "expect_long")
    t["EXPECT_LONG"] = t["SORT_LDS_MAX"] + t["SORT_LDS_MAX"] // int(m.group(1)) + int(m.group(2))
    body = _find(com, r"(?s)hgs_cell_class\(uint32_t len\) \{(.*?)\n\}", "hgs_cell_class").group(1)
    _find(body, r"nb = \(len \+ HGS_RB - 1\) / HGS_RB;", "batches of a cell list")
    t["CLASS_NB"] = [(int(a), int(b)) for a, b in re.findall(r"nb >= (\d+)u \? (\d+)u", body)]
    t["CLASS_REST"] = int(_find(body, r": (\d+)u - nb;", "the short classes").group(1))
    return t


def cell_class(t, length):
    """csrc/hgs_common.h: hgs_cell_class, restated from the parsed thresholds"""
    nb = (length + t["RB"] - 1) // t["RB"]
    for lo, cls in t["CLASS_NB"]:
        if nb >= lo:
            return cls
    return t["CLASS_REST"] - nb


def class_edges(t):
    """lengths L such that a cell list of L and one of L + 1 fall into different forward length classes"""
    top = t["RB"] * (max(lo for lo, _ in t["CLASS_NB"]) + 2)
    return [L for L in range(1, top) if cell_class(t, L) != cell_class(t, L + 1)]


def rank_nb(t, n):
    nb = t["NB_MIN"]
    while nb < t["NB_FACTOR"] * n and nb < t["NB_MAX"]:
        nb <<= 1
    return nb


def largest_bucket(t, depths, large_class):
    """csrc/binning.hip, steps 2-3 of the rank sort restated in fp32: the largest bucket of a tile list with these depths"""
    f = np.float32
    d = np.asarray(depths, f)
    nb = t["NB_MAX"] if large_class else rank_nb(t, len(d))
    lo, rng = d.min(), f(d.max() - d.min())
    scale = f(nb) / rng if rng > 1e-30 else f(0)
    b = np.minimum((d - lo).astype(f) * scale, f(nb - 1)).astype(np.uint32)
    return int(np.bincount(b, minlength=nb).max())
