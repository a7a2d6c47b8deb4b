"""The list pipeline - `hgs_k_sort_*`, the cell lists, `hgs_k_render_fwd_*`, `hgs_k_render_bwd`, `hgs_k_pair_reduce_{em,ch}` -
swept over every length at which it changes its code form, against the oracle, on scenes whose tile-list and cell-list
lengths are prescribed (tests/listscene.py), at N and at N + 1.

Tile-list length n:  multiples of HGS_CHUNK_RECS (64-record chunks, byte counters, chunk-cell-major pair ids); NB of the
rank sort doubling while NB < 2n up to HGS_RANK_NB_MAX (n = 128, 256, 512, 1024: bucket_scan's PER = 1, 2, 4, 8);
HGS_SORT_NT (a thread's second key); 2, 4, 8 x NT (rank_keys<2> / <4> / <8> / rank_keys_stream; the record rounds of
HGS_RANK_GU x NT and their hb / ha logic); HGS_SORT_LDS_MAX (hgs_k_sort_lds / hgs_k_sort_large); `expect_long` of api.hip
(6208: caller's stream / side stream); 16384 (hgs_k_sort_large / hgs_k_sort_huge); a bucket of HGS_RANK_BUCKET_MAX keys
(rank sort / bitonic fallback).  Cell-list length c:  HGS_RB (one staged batch or two); multiples of HGS_SEGLEN (stored
pixel state, backward work items); HGS_FWD_C4 (four cells per wave / one cell per wave, four records per iteration); the
edges of the forward's HGS_NFC length classes.  The lengths come from `listscene.thresholds()`, which parses the sources:
moving a threshold moves the cases (tests/test_list_boundaries_cpu.py checks that every threshold has its N and N + 1, and
every scene on the oracle alone).

Every case first asserts from `hgs_status` alone that it is the case it claims to be (longest list, entries, pairs: a dot is
one pair, a blanket 16), then the project's gates: radii == fp32 oracle; n_contrib == fp32 oracle per pixel except where
the oracle flags the pixel fragile; images within 1e-4; gradients within 1e-3 of max|g64| and cosine >= 1 - 1e-5 against the
fp64 oracle (flip Gaussians by the rule of helpers.check_against_fp64_oracle); in the thin regime, where every entry
matters, |got - g64| <= 0.25 |g64| on every opacity gradient of at least 1e-3 of the maximum - a dropped or doubled entry
is off by 1.0 there, the fp32 oracle by 1e-5."""
import types

import numpy as np
import pytest
import torch

import listscene as LS
from abi_runner import RawCall
from helpers import check_against_fp64_oracle, oracle_settings
from listscene import BLANKET, spec, spread

pytestmark = pytest.mark.gpu
IMG_TOL, GRAD_TOL, COS_TOL = 1e-4, 1e-3, 1e-5
PRESENCE_MIN, PRESENCE_TOL = 1e-3, 0.25
FRAGILE_CAP, FLIP_CAP = 0.02, 0.005            # of the pixels / of P (checked on the reference: test_list_boundaries_cpu.py)

T = LS.thresholds()
NT, LDS_MAX, HUGE = T["NT"], T["SORT_LDS_MAX"], T["HUGE"]


def regime_of(counts, ties=0):
    """What a scene of these cell counts can claim (listscene's docstring), by its fullest cell: thin up to 400 dots in a cell
    (fainter from 258 on, so that T stays >= 0.05), thick from THICK_MIN on, plain between and for ties (whose copies share
    one pixel, which must terminate INSIDE the group for n_contrib to depend on its order)."""
    m = max(n for (_, _, c), n in counts.items() if c != BLANKET)
    if ties:
        return dict(regime="plain", op=(0.03, 0.2), jitter=0.5)
    if m <= 2 * T["SEGLEN"] + 1:
        return dict(regime="thin", op=(0.01, 0.025), jitter=0.5)
    if m <= 400:
        return dict(regime="thin", op=(0.009, 0.018), jitter=0.5)
    if m >= LS.THICK_MIN:
        return dict(regime="thick", op=(0.05, 0.13), jitter=0.75)
    return dict(regime="plain", op=(0.03, 0.2), jitter=0.5)



def _pm(values):
    return sorted({v + d for v in values for d in (-1, 0, 1) if v + d >= 1})


# ---- a. tile-list lengths: N - 1, N, N + 1 around every switch, one more multiple of the chunk in every NB regime
def tile_lengths():
    nb_switch, nb = [], T["NB_MIN"]
    while nb < T["NB_MAX"]:                    # the n at which NB < NB_FACTOR * n first holds: NB doubles at n + 1
        nb_switch.append(nb // T["NB_FACTOR"])
        nb <<= 1
    forms = [NT] + [k * NT for k in T["KEYS_PER_THREAD"]] + [T["EARLY"] * NT]
    out = set(_pm([T["CHUNK_RECS"]] + nb_switch + forms + [LDS_MAX, HUGE])) | {1, T["EXPECT_LONG"], T["EXPECT_LONG"] + 1}
    for r in range(T["GU"] * NT, LDS_MAX, T["GU"] * NT):       # the record rounds of GU x NT keys (hb / ha): r rounds, r rounds + 1 key
        out |= {r, r + 1}
    regimes = sorted(set(nb_switch + forms + [LDS_MAX]))
    for lo, hi in zip(regimes, regimes[1:]):   # the last multiple of the chunk below the regime's end
        out.add(hi - T["CHUNK_RECS"])
    return sorted(out)


# Seeds picked so that the REFERENCE stays inside the caps of tests/test_list_boundaries_cpu.py (fragile pixels <= 2 % of the
# pixels, flip Gaussians <= 0.5 % of P: below 200 Gaussians that is none at all); the device's results are not consulted.
TILE_SEEDS = {HUGE: 21}
BLANKET_SEEDS = {64: 20, 65: 20, 256: 5}


def tile_scene(n):
    return spec(f"tile{n}", spread(n), seed=TILE_SEEDS.get(n, 0), **regime_of(spread(n)))


TILE_CASES = [tile_scene(n) for n in tile_lengths()]

# ---- c. degenerate depths at the bucket limit
DEGENERATE_N = [2 * NT, T["EARLY"] * NT + 1, 5000]
DEGENERATE_CASES = ([spec(f"ties{k}in{n}", spread(n), ties=k, seed=3, **regime_of(spread(n), ties=k))
                     for n in DEGENERATE_N for k in (T["BUCKET_MAX"], T["BUCKET_MAX"] + 1)]
                    + [spec(f"outlier{n}", spread(n), outlier=True, seed=4, **regime_of(spread(n)))
                       for n in DEGENERATE_N])

# ---- d. cell-list lengths: all dots of the tile in ONE cell; the regime by the length (regime_of)
CELL = 6
CELL_SEEDS = {}


def cell_lengths():
    seg, rb = T["SEGLEN"], T["RB"]
    c4 = rb * min(lo for lo, cls in T["CLASS_NB"] if cls < T["FWD_C4"])       # 208: the first length of 13 batches ...
    out = set(_pm([rb, seg, 2 * seg, 3 * seg, 4 * seg, c4 - rb, c4])) | {1, 8 * seg, 8 * seg + 1, LDS_MAX}
    for L in LS.class_edges(T):
        out |= {L, L + 1}
    return sorted(out)


def cell_scene(c):
    return spec(f"cell{c}", {(0, 0, CELL): c}, seed=CELL_SEEDS.get(c, 1), **regime_of({(0, 0, CELL): c}))


CELL_CASES = [cell_scene(c) for c in cell_lengths()]
C4_LAST = T["RB"] * (min(lo for lo, cls in T["CLASS_NB"] if cls < T["FWD_C4"]) - 1)      # 192: the longest four-cells-per-wave list


def _four_cells(name, a, b, c, d):
    counts = {(0, 0, 5): a, (0, 0, 6): b, (0, 0, 9): c, (0, 0, 10): d}
    return spec(name, counts, seed=2, **regime_of(counts))


MIXED_CELL_CASES = ([_four_cells(f"cells{L}_{L}_{L + 1}_{L + 1}", L, L, L + 1, L + 1) for L in LS.class_edges(T)]
                    + [_four_cells("cells_c4_switch", C4_LAST - 1, C4_LAST, C4_LAST + 1, C4_LAST + T["RB"] + 1)])

# ---- e. blankets: 16 pairs per entry
BLANKET_CASES = [spec(f"blankets{n}", {(0, 0, BLANKET): n}, regime="thin", seed=BLANKET_SEEDS[n]) for n in (64, 65, 256)]
MIXED_TILE = spec("blankets100_dots1000", {**spread(1000), (0, 0, BLANKET): 100}, seed=6, **regime_of(spread(1000)))

# ---- f. several classes in one call: nine tiles, dots in the four inner cells (their 3-sigma boxes stay inside the tile, so
# upstream's lists - the oracle's - and the device's are the same)
INNER = (5, 6, 9, 10)
NINE = [0, 1, 64, 2 * NT + 1, T["EARLY"] * NT + 1, LDS_MAX, LDS_MAX + 1, HUGE + 1, 300]


def _nine_tiles():
    counts = {}
    for i, n in enumerate(NINE):
        counts.update(spread(n, INNER, tile=(i % 3, i // 3)))
    return spec("nine_tiles", counts, H=48, W=48, seed=7, **regime_of(counts))


NINE_TILES = _nine_tiles()

# ---- g. three views
THREE_VIEW_CASES = ([tile_scene(n) for n in (T["CHUNK_RECS"], T["CHUNK_RECS"] + 1, LDS_MAX, LDS_MAX + 1)]
                    + [MIXED_CELL_CASES[-1], MIXED_TILE])

ALL_SCENES = (TILE_CASES + DEGENERATE_CASES + CELL_CASES + MIXED_CELL_CASES + BLANKET_CASES + [MIXED_TILE, NINE_TILES])


def sid(sp):
    return sp.name


# ------------------------------------------------------------------------------------------------- running and gating
def run_forward(sp, hint=0):
    sc = LS.scene(sp)
    rc = RawCall(sc, capacity=max(64, 2 * sc["means3D"].shape[0]), max_tile_hint=hint, mapped=1)
    assert rc.forward() == 0
    return rc


def assert_is_the_case(sp, rc):
    """from hgs_status alone: longest list, entries, pairs"""
    lists = LS.prescribed_lists(sp)
    assert rc.status[4] == 0, ("overflow", rc.status)
    assert rc.status[6] == max(lists.values()), ("longest list", rc.status[6], max(lists.values()))
    assert rc.status[0] == sum(lists.values()), ("entries", rc.status[0], sum(lists.values()))
    assert rc.status[1] == len(lists), ("active tiles", rc.status[1], len(lists))
    assert rc.status[2] == LS.prescribed_pairs(sp), ("pairs: a dot is one, a blanket 16", rc.status[2], LS.prescribed_pairs(sp))


def n_contrib_of(rc):
    return torch.from_numpy(np.frombuffer(rc.img[: rc.H * rc.W * 4].cpu().numpy().tobytes(), dtype=np.uint32)
                            .astype(np.int64).reshape(rc.H, rc.W))


def check_images(color, depth, alpha, o32, what):
    """tests/test_gpu_parity.py: check_images"""
    dmax = max(1.0, float(o32["depth"].max()))
    for k, got, tol in (("color", color, IMG_TOL), ("alpha", alpha, IMG_TOL), ("depth", depth, IMG_TOL * dmax)):
        assert torch.isfinite(got).all(), (what, k, "non-finite")
        err = float((got.cpu().double() - o32[k].double()).abs().max())
        print(f"{what}: {k} err {err:.2e}")
        assert err <= tol, (what, k, err)


def check_forward(sp, rc):
    o32, _ = LS.reference(sp)
    assert torch.equal(rc.radii.cpu(), o32["radii"]), (sp.name, "radii")
    nc = n_contrib_of(rc)
    solid = ~o32["fragile"]
    assert torch.equal(nc[solid], o32["n_contrib"][solid]), (sp.name, "n_contrib", int((nc != o32["n_contrib"])[solid].sum()))
    check_images(rc.color, rc.depth, rc.alpha, o32, sp.name)


def check_gradients(sp, images, grads, o32, o64, upstream, what):
    """`grads`: dict of CPU tensors, means2D (P, 3).  helpers.check_against_fp64_oracle with the scene's cached references:
    non-flip Gaussians within 1e-3 of max|g64| (and of the fp32 oracle), cosine >= 1 - 1e-5, flip Gaussians by its rule;
    the caps on fragile pixels and flip Gaussians are the ones of tests/test_list_boundaries_cpu.py."""
    sc = LS.scene(sp)
    P = sc["means3D"].shape[0]
    flip = o32["flip_gaussians"] | o64["flip_gaussians"]
    assert int(o32["fragile"].sum()) <= FRAGILE_CAP * sp.H * sp.W and int(flip.sum()) <= FLIP_CAP * P, (what, "caps of the reference")
    got = {k: v for k, v in grads.items() if v is not None}
    assert set(got) == set(o64["grads"]), (set(got), set(o64["grads"]))
    for k, g in got.items():
        assert torch.isfinite(g).all(), (what, k, "non-finite", int((~torch.isfinite(g)).sum()))
    cloud = types.SimpleNamespace(means3D=sc["means3D"], shs=sc["shs"], opacities=sc["opacities"], scales=sc["scales"],
                                  rotations=sc["rotations"])
    color, radii, depth, alpha = images
    check_against_fp64_oracle(what, cloud, oracle_settings(sc), (color, radii, depth, alpha, got), upstream, img_tol=IMG_TOL,
                              grad_tol=GRAD_TOL, cos_tol=COS_TOL, threads=16, minority_caps=False, refs=(o32, o64))
    if sp.regime == "thin":                                  # presence: every entry that matters is there once
        ref = o64["grads"]["opacities"].reshape(-1)
        g = got["opacities"].double().reshape(-1)
        sel = ref.abs() >= PRESENCE_MIN * float(ref.abs().max())
        assert int(sel.sum()) > 0
        worst = float(((g - ref).abs() / ref.abs())[sel].max())
        print(f"{what}: presence: {int(sel.sum())} of {P} Gaussians, worst relative error {worst:.2e}")
        assert worst <= PRESENCE_TOL, (what, "an entry is missing or counted twice", worst)


def run_and_check(sp, hint=0, pairs_scratch=False):
    rc = run_forward(sp, hint)
    assert_is_the_case(sp, rc)
    check_forward(sp, rc)
    o32, o64 = LS.reference(sp)
    up = LS.upstream(sp)
    grads = rc.backward(*up, pairs_scratch=pairs_scratch)
    check_gradients(sp, (rc.color.cpu(), rc.radii.cpu(), rc.depth.cpu(), rc.alpha.cpu()), grads, o32, o64, up, sp.name)
    return rc, grads


def bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def assert_same_bits(ra, ga, rb, gb, what):
    for k in ("color", "depth", "alpha", "radii"):
        assert bitwise(getattr(ra, k), getattr(rb, k)), (what, k)
    assert torch.equal(n_contrib_of(ra), n_contrib_of(rb)), (what, "n_contrib")
    for k in ga:
        if ga[k] is not None:
            assert bitwise(ga[k], gb[k]), (what, k, float((ga[k] - gb[k]).abs().max()))


# ------------------------------------------------------------------------------------------------- a. tile-list boundaries
@pytest.mark.parametrize("sp", TILE_CASES, ids=sid)
def test_tile_list_length(sp):
    run_and_check(sp)


# ------------------------------------------------------------------------------------------------- b. class routing by the hint
def test_hint_routes_the_large_class():
    sp = tile_scene(LDS_MAX + 1)
    over = run_forward(sp, hint=LDS_MAX)
    assert over.status[4] & 2 and over.status[6] == LDS_MAX + 1        # the broken promise is reported, with the longest list
    base, gbase = run_and_check(sp, hint=0)
    for hint in (LDS_MAX + 1, T["EXPECT_LONG"] + 1):                    # large class on the caller's stream / on the side stream
        rc, g = run_and_check(sp, hint=hint)
        assert_same_bits(base, gbase, rc, g, ("hint", hint))


def test_hint_routes_the_huge_class():
    sp = tile_scene(HUGE + 1)
    over = run_forward(sp, hint=HUGE)
    assert over.status[4] & 2 and over.status[6] == HUGE + 1
    base, gbase = run_and_check(sp, hint=0)
    rc, g = run_and_check(sp, hint=HUGE + 1)
    assert_same_bits(base, gbase, rc, g, ("hint", HUGE + 1))


def test_hint_equal_to_the_longest_list_is_kept():
    sp = tile_scene(LDS_MAX)
    rc, _ = run_and_check(sp, hint=LDS_MAX)
    assert rc.status[4] == 0


# ------------------------------------------------------------------------------------------------- c. degenerate depths
@pytest.mark.parametrize("sp", DEGENERATE_CASES, ids=sid)
def test_degenerate_depths_at_the_bucket_limit(sp):
    run_and_check(sp)


# ------------------------------------------------------------------------------------------------- d. cell-list boundaries
@pytest.mark.parametrize("sp", CELL_CASES + MIXED_CELL_CASES, ids=sid)
def test_cell_list_length(sp):
    run_and_check(sp)


# ------------------------------------------------------------------------------------------------- e. blankets
@pytest.mark.parametrize("sp", BLANKET_CASES + [MIXED_TILE], ids=sid)
def test_blankets_reach_every_cell(sp):
    rc, _ = run_and_check(sp, pairs_scratch=True)          # (RawCall.backward asserts the guard bytes behind the scratch)
    n_blankets = sum(n for (_, _, c), n in sp.counts if c == BLANKET)
    assert rc.status[2] == T["PAIRS_PER_ENTRY"] * n_blankets + (rc.status[0] - n_blankets)


# ------------------------------------------------------------------------------------------------- f. several classes in one call
def test_nine_tiles_of_every_sort_class_in_one_call():
    sp = NINE_TILES
    assert sorted(LS.prescribed_lists(sp).values()) == sorted(n for n in NINE if n)
    a, ga = run_and_check(sp, hint=0)
    b, gb = run_and_check(sp, hint=0)
    assert_same_bits(a, ga, b, gb, "second run")


# ------------------------------------------------------------------------------------------------- g. three views
def _batch(sp, views):
    from humangaussian_amd import GaussianRasterizationSettings, rasterize_gaussians_batch
    import math
    sc, dev = LS.scene(sp), "cuda"
    cam = sc["cam"]
    rs = GaussianRasterizationSettings(sp.H, sp.W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), sc["bg"].to(dev), 1.0,
                                       cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 0,
                                       cam.camera_center.to(dev), False, False)
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    ins = {k: sc[k].to(dev).requires_grad_(True) for k in names}
    B, P = len(views), sc["means3D"].shape[0]
    m2 = torch.zeros(B, P, 3, device=dev, requires_grad=True)
    color, radii, depth, alpha = rasterize_gaussians_batch(ins["means3D"], m2, ins["shs"], None, ins["opacities"], ins["scales"],
                                                           ins["rotations"], None, [rs] * B)
    ups = [LS.upstream(sp, v) for v in views]
    gouts = [torch.stack([u[i] for u in ups]).to(dev) for i in range(3)]
    gl = torch.autograd.grad([color, depth, alpha], list(ins.values()) + [m2], gouts)
    torch.cuda.synchronize()
    return dict(color=color.detach().cpu(), depth=depth.detach().cpu(), alpha=alpha.detach().cpu(), radii=radii.cpu(),
                grads={k: g.detach().cpu() for k, g in zip(names + ("means2D",), gl)})


@pytest.mark.parametrize("sp", THREE_VIEW_CASES, ids=sid)
def test_three_views_chunk_cell_major_rows(sp):
    assert_is_the_case(sp, run_forward(sp))      # (the torch binding hands out no status: the lengths of the same scene through the raw ABI)
    views = [0, 1, 2]
    refs = [LS.reference(sp, v) for v in views]
    r = _batch(sp, views)
    singles = [_batch(sp, [v]) for v in views]
    for b, (o32, o64) in enumerate(refs):
        assert torch.equal(r["radii"][b], o32["radii"])
        check_images(r["color"][b], r["depth"][b], r["alpha"][b], o32, f"{sp.name} view {b}")
        for k in ("color", "depth", "alpha", "radii"):
            assert bitwise(r[k][b], singles[b][k][0]), (b, k)
        assert bitwise(r["grads"]["means2D"][b], singles[b]["grads"]["means2D"][0]), b
    for k in r["grads"]:                                     # the contract: three single calls summed in view order
        if k != "means2D":
            want = singles[0]["grads"][k].clone()
            for s in singles[1:]:
                want += s["grads"][k]
            assert bitwise(r["grads"][k], want), (k, float((r["grads"][k] - want).abs().max()))
    # the summed gradients against the sum of the three oracle backwards; means2D per view against its own
    o32s, o64s = ({**refs[0][i], "grads": {k: sum(rf[i]["grads"][k] for rf in refs) for k in refs[0][i]["grads"]}} for i in (0, 1))
    ups = [sum(LS.upstream(sp, v)[i] for v in views) for i in range(3)]
    summed = dict(r["grads"], means2D=r["grads"]["means2D"].double().sum(0).float())
    check_gradients(sp, (r["color"][0], r["radii"][0], r["depth"][0], r["alpha"][0]), summed, o32s, o64s, ups, f"{sp.name} three views")
    for b, (o32, o64) in enumerate(refs):
        ref = o64["grads"]["means2D"]
        err = float((r["grads"]["means2D"][b].double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
        assert err <= GRAD_TOL, (b, "means2D", err)
