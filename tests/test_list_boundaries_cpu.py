"""CPU companion of tests/test_gpu_list_boundaries.py: keeps its case table and its scenes honest, on the reference alone.

1. The table.  The thresholds of the list pipeline are parsed out of the sources (`listscene.thresholds()`: a threshold that
   can no longer be found fails); every one of them must have a case at N and at N + 1, the forward's length classes are
   restated (`listscene.cell_class`) and every class edge L must appear as L and L + 1 among the cell-list cases.
2. Every scene of the GPU module: the oracle's tile lists have exactly the prescribed lengths; by fp64 brute force over
   the pixel centres every dot's live pixels (alpha >= 1/255) lie in its one cell and there is at least one, every
   blanket has a live pixel in all 16 cells; the device's own mask and rect functions (csrc/cellmask.h compiled for the
   host) give a dot exactly its cell's bit, a blanket all 16, and either exactly its tile; thin scenes keep T >= 0.05
   everywhere; in every cell of at least THICK_MIN dots of a thick scene more than half of the 16 pixels terminate inside
   the list, at cell-list positions in at least three 128-entry segments (plain scenes claim neither; in a tie scene a
   pixel under the copies terminates inside the group, whose order is the Gaussian index); the fp32 oracle's gradients are within 2.5e-4 of max|g64| per
   tensor (the margin of tests/test_pre_bwd_matrix_cpu.py: the GPU module's 1e-3 then tests the kernel, not fp32);
   fragile pixels are at most 2 % of the pixels and flip Gaussians at most 0.5 % of P.  Tie scenes: the k copies fill a
   bucket of the rank sort alone (192: rank sort, 193: bitonic fallback); outlier scenes overflow a bucket."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import listscene as LS
import oracle
import test_gpu_list_boundaries as G
from helpers import oracle_settings
from listscene import BLANKET

T = G.T
ORACLE_TOL = 0.25 * G.GRAD_TOL


# ------------------------------------------------------------------------------------------------- 1. the table
def test_every_threshold_is_found_and_has_the_expected_value_kinds():
    assert T["NB_MIN"] == T["NT"] and T["NB_MAX"] == T["EARLY"] * T["NT"]            # bucket_scan: PER = NB / NT = 1 .. 8
    assert T["KEYS_PER_THREAD"] == [2, 4] and T["EARLY"] == 8
    assert T["SORT_LDS_MAX"] == 16 * T["NT"] and T["HUGE"] > T["SORT_LDS_MAX"]
    assert T["SORT_LDS_MAX"] < T["EXPECT_LONG"] < T["HUGE"]
    assert T["CLASS_REST"] == T["NFC"] and min(lo for lo, _ in T["CLASS_NB"]) - 1 + len(T["CLASS_NB"]) == T["NFC"]   # 7 classes by thresholds + 1 .. 4 batches
    assert sorted({LS.cell_class(T, n) for n in range(1, 1000)}) == list(range(T["NFC"]))
    assert T["BUCKET_MAX"] < 256 and T["PAIRS_PER_ENTRY"] == 16


def test_every_tile_list_threshold_has_n_and_n_plus_1():
    have = {sum(n for _, n in sp.counts) for sp in G.TILE_CASES}
    need = {"chunk": T["CHUNK_RECS"], "second key": T["NT"], "rank_keys<2>": 2 * T["NT"], "rank_keys<4>": 4 * T["NT"],
            "stream form": T["EARLY"] * T["NT"], "large class": T["SORT_LDS_MAX"], "side stream": T["EXPECT_LONG"],
            "huge class": T["HUGE"]}
    nb = T["NB_MIN"]
    while nb < T["NB_MAX"]:
        need[f"NB {nb} -> {2 * nb}"] = nb // T["NB_FACTOR"]
        assert LS.rank_nb(T, nb // T["NB_FACTOR"]) == nb and LS.rank_nb(T, nb // T["NB_FACTOR"] + 1) == 2 * nb
        nb <<= 1
    missing = [k for k, n in need.items() if not {n, n + 1} <= have]
    assert not missing, missing
    # the record rounds of HGS_RANK_GU * NT keys (hb / ha): a list of exactly r rounds, and one more key, up to the class's end
    per_round = T["GU"] * T["NT"]
    for r in range(1, T["SORT_LDS_MAX"] // per_round + 1):
        assert {r * per_round, r * per_round + 1} <= have, r
    ends = sorted(set(need[k] for k in need if k.startswith("NB")) | {2 * T["NT"], 4 * T["NT"], T["EARLY"] * T["NT"], T["SORT_LDS_MAX"]})
    for lo, hi in zip(ends, ends[1:]):                                                        # one more multiple of the chunk per regime
        assert any(lo < n < hi - 1 and n % T["CHUNK_RECS"] == 0 for n in have), (lo, hi)
    # (the issue's own list, literally: what the derivation above must contain at today's constants)
    assert {1, 63, 64, 65, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6208,
            6209, 16383, 16384, 16385, 192, 448, 960, 1984, 4032} <= have
    assert all(len(sp.counts) == min(16, n) for sp in G.TILE_CASES for n in [sum(k for _, k in sp.counts)])   # spread over the cells


def test_every_cell_list_threshold_and_class_edge_has_l_and_l_plus_1():
    have = {n for sp in G.CELL_CASES for _, n in sp.counts}
    edges = LS.class_edges(T)
    assert len(edges) == T["NFC"] - 1, edges
    assert edges == [T["RB"] * (nb - 1) for nb in sorted({lo for lo, _ in T["CLASS_NB"]} | set(range(2, T["CLASS_REST"] - len(T["CLASS_NB"]) + 1)))], edges
    for L in edges + [T["RB"], T["SEGLEN"], 2 * T["SEGLEN"], 3 * T["SEGLEN"], 4 * T["SEGLEN"], 8 * T["SEGLEN"], G.C4_LAST,
                      G.C4_LAST + T["RB"]]:
        assert {L, L + 1} <= have, L
    assert LS.cell_class(T, G.C4_LAST) >= T["FWD_C4"] > LS.cell_class(T, G.C4_LAST + 1)          # 192 / 193
    assert {1, 15, 16, 17, 127, 128, 129, 191, 192, 193, 207, 208, 209, 255, 256, 257, 383, 384, 385, 511, 512, 513, 1024, 1025,
            4096} <= have                                        # (the issue's own list, literally)
    mixed = [tuple(n for _, n in sp.counts) for sp in G.MIXED_CELL_CASES]
    assert all((L, L, L + 1, L + 1) in mixed for L in edges) and (191, 192, 193, 209) in mixed
    assert all(len({LS.cell_class(T, n) for n in m}) == 2 for m in mixed[:-1])


def test_every_scene_claims_what_its_fullest_cell_allows():
    by = {r: [sp.name for sp in G.ALL_SCENES if sp.regime == r] for r in ("thin", "thick", "plain")}
    assert {"cell4096", "nine_tiles"} == set(by["thick"]), by["thick"]      # (1024 dots in a cell terminate only the four central pixels)
    assert all(sp.regime == "thin" for sp in G.TILE_CASES if sum(n for _, n in sp.counts) <= T["EXPECT_LONG"] + 1)
    assert all(sp.regime == "thin" for sp in G.CELL_CASES if sp.counts[0][1] <= 2 * T["SEGLEN"] + 1)       # short cell lists: presence gate
    assert all(sp.regime == "plain" for sp in G.ALL_SCENES if sp.ties)


def test_the_other_sections_hold_their_cases():
    names = {sp.name for sp in G.ALL_SCENES}
    assert len(names) == len(G.ALL_SCENES)
    assert {"ties192in512", "ties193in512", "ties192in2049", "ties193in2049", "ties192in5000", "ties193in5000", "outlier512",
            "outlier2049", "outlier5000", "blankets64", "blankets65", "blankets256", "blankets100_dots1000"} <= names
    assert sorted(LS.prescribed_lists(G.NINE_TILES).values()) == sorted([1, 64, 513, 2049, 4096, 4097, 16385, 300])
    assert [sum(n for _, n in sp.counts) for sp in G.THREE_VIEW_CASES[:4]] == [64, 65, 4096, 4097]
    assert all(sp in G.ALL_SCENES for sp in G.THREE_VIEW_CASES)


# ------------------------------------------------------------------------------------------------- 2. the scenes
@pytest.fixture(scope="module")
def cellmask(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cellmask") / "cellmask_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           os.path.join(LS.ROOT, "tests", "cellmask_host.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hgs_cell_mask_host.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 9
    lib.hgs_alpha_rect_host.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 7
    return lib


def _pre(sc, dtype):
    with torch.no_grad():
        return oracle.preprocess(sc["means3D"], None, sc["shs"], None, sc["opacities"], sc["scales"], sc["rotations"], None,
                                 oracle_settings(sc), dtype)


def _live_cells(sp, pre):
    """fp64 brute force: (P, tiles * 16) bool - Gaussian i has a live pixel centre in cell c of tile t"""
    gx = (sp.W + 15) // 16
    ys, xs = torch.meshgrid(torch.arange(sp.H), torch.arange(sp.W), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    slot = ((ys // 16) * gx + xs // 16) * 16 + ((ys % 16) // 4) * 4 + (xs % 16) // 4
    P = pre["mean2D"].shape[0]
    out = torch.zeros(P, gx * ((sp.H + 15) // 16) * 16, dtype=torch.bool)
    for s in range(0, P, 4096):
        m, con, op = pre["mean2D"][s:s + 4096], pre["conic"][s:s + 4096], pre["opacity"][s:s + 4096]
        dx, dy = m[:, 0:1] - xs[None].double(), m[:, 1:2] - ys[None].double()
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        live = (power <= 0) & (op[:, None] * torch.exp(power) >= 1.0 / 255.0)
        out[s:s + 4096] = torch.zeros(live.shape[0], out.shape[1], dtype=torch.int32).index_add_(
            1, slot, live.to(torch.int32)) > 0
    return out


@pytest.mark.parametrize("sp", G.ALL_SCENES, ids=G.sid)
def test_scene_on_the_reference_alone(sp, cellmask):
    sc = LS.scene(sp)
    P = sc["means3D"].shape[0]
    kind, cell, tile = sc["kind"], sc["cell"], sc["tile"]
    pre32, pre64 = _pre(sc, torch.float32), _pre(sc, torch.float64)
    # the target pixel positions, and the prescribed tile lists
    assert float((pre64["mean2D"] - sc["target"].double()).abs().max()) < (1e-3 if sp.outlier else 2e-5)
    _, _, ranges = oracle.bin_and_sort(pre32)
    lengths = {t: int(n) for t, n in enumerate((ranges[:, 1] - ranges[:, 0]).tolist()) if n}
    assert lengths == LS.prescribed_lists(sp), (lengths, LS.prescribed_lists(sp))
    # one cell per dot, sixteen per blanket: fp64 brute force, then the device's own functions on the fp32 values
    live = _live_cells(sp, pre64)
    want = torch.zeros_like(live)
    dots = kind == 0
    want[torch.nonzero(dots).reshape(-1), (tile * 16 + cell)[dots]] = True
    for c in range(16):
        want[torch.nonzero(~dots).reshape(-1), tile[~dots] * 16 + c] = True
    assert torch.equal(live, want), ("live pixels outside the cell, or none", int((live != want).any(1).sum()))
    f = lambda t: np.ascontiguousarray(t.numpy(), np.float32)  # noqa: E731
    gx = (sp.W + 15) // 16
    arrs = [f(pre32["mean2D"][:, 0]), f(pre32["mean2D"][:, 1]), f(pre32["conic"][:, 0]), f(pre32["conic"][:, 1]),
            f(pre32["conic"][:, 2]), f(pre32["opacity"])]
    x0, y0 = f((tile % gx) * 16.0), f((tile // gx) * 16.0)
    masks = np.zeros(P, np.uint32)
    cellmask.hgs_cell_mask_host(P, *[a.ctypes.data for a in arrs], x0.ctypes.data, y0.ctypes.data, masks.ctypes.data)
    expect = np.where(kind.numpy() == 1, 0xffff, 1 << np.maximum(cell.numpy(), 0)).astype(np.uint32)
    assert np.array_equal(masks, expect), ("the cell mask", int((masks != expect).sum()))
    rect = np.ascontiguousarray(pre32["rect"].numpy(), np.int32)
    cellmask.hgs_alpha_rect_host(P, *[a.ctypes.data for a in arrs], rect.ctypes.data)
    tx, ty = (tile % gx).numpy(), (tile // gx).numpy()
    assert np.array_equal(rect, np.stack([tx, ty, tx + 1, ty + 1], 1)), "the cut tile rect"
    # the oracle: regime, fp32 against fp64, caps
    views = (0, 1, 2) if sp in G.THREE_VIEW_CASES else (0,)
    for v in views:
        o32, o64 = LS.reference(sp, v)
        assert o32["max_list"] == max(lengths.values()) and o32["num_rendered"] == P
        for k, ref in o64["grads"].items():
            err = float((o32["grads"][k].double().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
            assert err <= ORACLE_TOL, (v, k, err)
    o32, o64 = LS.reference(sp)
    flip = o32["flip_gaussians"] | o64["flip_gaussians"]
    assert int(o32["fragile"].sum()) <= G.FRAGILE_CAP * sp.H * sp.W, int(o32["fragile"].sum())
    assert int(flip.sum()) <= G.FLIP_CAP * P, (int(flip.sum()), P)
    t_final = 1.0 - o64["alpha"][0]
    g_sorted, _, _ = oracle.bin_and_sort(pre32)
    gx = (sp.W + 15) // 16
    if sp.regime == "thin":
        assert float(t_final.min()) >= 0.05, float(t_final.min())
        ref = o64["grads"]["opacities"].reshape(-1)                  # the presence gate has something to look at, and the fp32
        sel = ref.abs() >= G.PRESENCE_MIN * float(ref.abs().max())   # oracle meets it by orders of magnitude
        assert int(sel.sum()) >= 0.25 * P
        assert float(((o32["grads"]["opacities"].double().reshape(-1) - ref).abs() / ref.abs())[sel].max()) <= 1e-3
    elif sp.regime == "thick":
        loaded = [(k, n) for k, n in sp.counts if n >= LS.THICK_MIN]
        assert loaded
        hi = max(sp.op)
        for (tX, tY, c), n in loaded:
            t = tY * gx + tX
            order = g_sorted[ranges[t, 0]:ranges[t, 1]]
            cellpos = torch.cumsum((cell[order] == c).long(), 0)     # cell-list position of the tile list's k-th entry
            y0, x0 = tY * 16 + (c // 4) * 4, tX * 16 + (c % 4) * 4
            nc = o64["n_contrib"][y0:y0 + 4, x0:x0 + 4].reshape(-1)
            done = (t_final[y0:y0 + 4, x0:x0 + 4].reshape(-1) < 1e-4 / (1 - hi)) & (nc > 0)   # (T in front of the stopper < 1e-4 / (1 - alpha))
            assert int(done.sum()) > 8, ((tX, tY, c), n, "pixels that terminate", int(done.sum()))
            stops = cellpos[nc[done] - 1]
            assert bool((stops < n).all())
            segs = sorted(set((stops // T["SEGLEN"]).tolist()))
            assert len(segs) >= 3, ((tX, tY, c), n, "segments with a terminating pixel", segs)
    if sp.ties:                                                      # the pixels under the copies stop INSIDE the group
        tied = torch.nonzero(pre32["depth"] == pre32["depth"].mode().values).reshape(-1)
        ranks = torch.nonzero(torch.isin(g_sorted, tied)).reshape(-1) + 1
        assert torch.equal(g_sorted[ranks - 1], tied), "ties are listed by Gaussian index"
        inside = (o64["n_contrib"] > int(ranks[0])) & (o64["n_contrib"] < int(ranks[-1]))
        assert int(inside.sum()) >= 1, "no pixel terminates inside the tied group"
    # degenerate depths: what the rank sort will see
    if sp.ties or sp.outlier:
        n = P
        big = LS.largest_bucket(T, pre32["depth"].numpy(), large_class=n > T["SORT_LDS_MAX"])
        if sp.ties:
            assert big == sp.ties, (big, sp.ties)                    # the copies have their bucket to themselves
            d = pre32["depth"]
            assert int((d == d.mode().values).sum()) == sp.ties
        else:
            assert big > T["BUCKET_MAX"] + T["BUCKET_MAX"] // 4, big
