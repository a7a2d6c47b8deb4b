"""CPU companion of tests/test_gpu_fields_forms.py: holds the case table (tests/fields_cases.py) to its claims on the numpy
restatement alone (tests/fields_reference.py).

1. The forms.  The constants are parsed out of csrc/fields.hip and csrc/api.hip (one that can no longer be found fails here);
   the splits of the table cover both workgroup sizes, one slab and several, odd and even splits, s = 1, both sides of the
   64-thread rule and of one slab, nb = 1, nb = HGS_FIELD_MAX_BLOCKS, an nb that is no power of two, and list lengths on
   both sides of one and of two HGS_FIELD_CHUNK.
2. The clouds.  (a) and (c) are all-listed and unflagged; the fp64 field of (a) does not depend on num_blocks; the seeds of (b)
   stay under the near-cut cap and their lists are what the cases claim; every record of (c) is visible; (d) keeps the same
   records scattered and compacted; (e) spans no extent; the refused dimensions break the integer rules, and the integer rule
   accepts what the reference's float assertion refused."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_cases as FC  # noqa: E402
import fields_reference as FR  # noqa: E402


def _splits():
    s = {res // nb for res, nbs in FC.A_TABLE.items() for nb in nbs}
    s |= {c[0] // c[1] for c in FC.B_CASES} | {res // nb for res, nb in FC.C_FORMS}
    return s


def test_constants_are_parsed_and_the_form_is_restated():
    c = FC.constants()
    assert set(c) == {"CHUNK", "MAX_BLOCKS", "MAX_SPLIT", "MAX_RES", "SMALL_ITEMS", "SMALL_THREADS", "THREADS"}
    assert all(isinstance(v, int) and v > 0 for v in c.values())
    assert c["SMALL_THREADS"] < c["THREADS"] and c["SMALL_ITEMS"] <= c["SMALL_THREADS"]      # no item without a thread
    assert c["MAX_BLOCKS"] == 32                                   # a block range is 2 x 5 bits per axis (fields.hip)
    for s in range(1, c["MAX_SPLIT"] + 1):
        items, threads, slabs, odd = FC.eval_form(s)
        # a thread owns xp and xp + ceil(s / 2): the items are the (xp, y, z) with xp < ceil(s / 2), and together with
        # their partners they are every sample of the block once - the middle plane of an odd split has no partner
        half = (s + 1) // 2
        assert items == half * s * s and odd == (2 * half != s)
        assert 2 * items - (s * s if odd else 0) == s ** 3
        assert threads in (c["SMALL_THREADS"], c["THREADS"]) and (slabs - 1) * threads < items <= slabs * threads
        assert (threads == c["SMALL_THREADS"]) == (items <= c["SMALL_ITEMS"])


def test_the_table_covers_every_form():
    c = FC.constants()
    splits = _splits()
    forms = {s: FC.eval_form(s) for s in splits}
    assert {f[1] for f in forms.values()} == {c["SMALL_THREADS"], c["THREADS"]}
    assert any(f[2] == 1 for f in forms.values()) and any(f[2] > 1 for f in forms.values())
    assert any(f[3] for f in forms.values()) and any(not f[3] for f in forms.values())
    assert any(f[3] and f[2] > 1 for f in forms.values())                     # an odd split of several slabs
    assert any(f[1] == c["THREADS"] and f[0] % c["THREADS"] for f in forms.values())      # a partly filled last workgroup
    assert {1, 2, 3} <= splits
    # either side of the 64-thread rule and of one slab: the last split below, the first above
    small = max(s for s in range(1, c["MAX_SPLIT"]) if FC.eval_form(s)[0] <= c["SMALL_ITEMS"])
    one = max(s for s in range(1, c["MAX_SPLIT"]) if FC.eval_form(s)[0] <= c["THREADS"])
    assert {small, small + 1, one, one + 1} <= splits
    assert (FC.eval_form(small)[0], FC.eval_form(small + 1)[0]) == (32, 75)
    assert (FC.eval_form(one)[0], FC.eval_form(one + 1)[0]) == (256, 405)
    assert FC.eval_form(one)[2] == 1 and FC.eval_form(one + 1)[2] == 2
    # every split of (a) is compared with the pinned one, which the existing suite holds to fp64 at 1.25 e
    for res, nbs in FC.A_TABLE.items():
        assert all(res % nb == 0 for nb in nbs) and res // FC.A_PINNED_SPLIT in nbs and res // 4 in nbs
    assert FC.A_GATED_RES in FC.A_TABLE
    # (b): the kinds of block count, with cut lists
    nbs = {case[1] for case in FC.B_CASES if case[2] == 1.5}
    assert 1 in nbs and c["MAX_BLOCKS"] in nbs and any(nb & (nb - 1) for nb in nbs)
    assert {case[0] // case[1] for case in FC.B_CASES if case[2] == 1.5} >= {1, 2, 3, 5, 7, 8, 9, 16}
    assert all(case[0] % case[1] == 0 and len(FC.cloud_b(case[3], case[4])[0]) <= 3000 for case in FC.B_CASES)
    assert all(case[3] <= 1500 for case in FC.B_CASES if case[0] // case[1] >= 16)
    assert sum(case[2] == 0.0 for case in FC.B_CASES) == 3
    # (c): both sides of one and of two chunks, in a 64-thread and in a 256-thread form of several slabs
    ks = FC.c_lengths()
    assert {c["CHUNK"] - 1, c["CHUNK"], c["CHUNK"] + 1, 2 * c["CHUNK"] - 1, 2 * c["CHUNK"], 2 * c["CHUNK"] + 1, 2} == set(ks)
    cf = [FC.eval_form(res // nb) for res, nb in FC.C_FORMS]
    assert {f[1] for f in cf} == {c["SMALL_THREADS"], c["THREADS"]} and any(f[2] > 1 for f in cf)
    # no shape beyond the limits
    for res, nb in [(r, n) for r, ns in FC.A_TABLE.items() for n in ns] + [case[:2] for case in FC.B_CASES] + FC.C_FORMS:
        assert 1 <= nb <= c["MAX_BLOCKS"] and res <= c["MAX_RES"] and res // nb <= c["MAX_SPLIT"]


def test_dead_rows_are_of_four_kinds_and_none_is_kept():
    xyz, op, _, _ = FC.dead(64, 3)
    assert len(FC.kept_rows(FC.dead(64, 3))[0]) == 0
    o = op.reshape(-1)
    kinds = [o == FR.OPACITY_CUT, o == 0, np.isnan(xyz).any(1), np.isinf(xyz).any(1)]
    assert len(FC.DEAD_KINDS) == 4 and all(k.sum() == 16 for k in kinds) and (np.sum(kinds, 0) == 1).all()
    assert (o[kinds[2] | kinds[3]] > 0.5).all()                     # only the coordinate keeps them out
    assert np.isposinf(xyz).any() and np.isneginf(xyz).any()
    fin = np.isfinite(xyz)
    assert (np.abs(xyz[fin]) >= 3).all()                            # far outside any kept cloud of the table
    for cloud in (FC.cloud_a(), FC.cloud_b(1500, 32), FC.cloud_c(257)):
        k = FC.kept_rows(cloud)
        assert np.abs(k[0]).max() < 1.5 and 0 < len(k[0]) < len(cloud[0])


@pytest.mark.parametrize("res", sorted(FC.A_TABLE))
def test_a_is_all_listed_and_its_fp64_field_does_not_depend_on_the_block_count(res):
    cloud = FC.cloud_a()
    kept = len(FC.kept_rows(cloud)[0])
    assert 350 < kept < len(cloud[0]) <= 420 and kept > FC.constants()["CHUNK"]
    nbs = FC.A_TABLE[res]
    for nb in nbs:
        P = FR.prepare(*cloud, res, nb, FC.all_listed(nb), np.float64)
        counts, flagged = FR.block_counts(P)
        assert (counts == kept).all() and not flagged.any(), nb
        assert float(np.abs(P.n).max()) <= 0.9 + 1e-12 and (P.lo < -1.9).all() and (P.hi > 1.9).all()
    lo = FR.field(*cloud, resolution=res, num_blocks=nbs[0], relax_ratio=FC.all_listed(nbs[0]), dtype=np.float64)[0]
    hi = FR.field(*cloud, resolution=res, num_blocks=nbs[-1], relax_ratio=FC.all_listed(nbs[-1]), dtype=np.float64)[0]
    assert lo.max() > 0.5 and np.array_equal(lo, hi)


@pytest.mark.parametrize("case", FC.B_CASES, ids=FC.b_id)
def test_b_seeds_stay_under_the_near_cut_cap_and_the_lists_are_what_the_case_claims(case):
    res, nb, relax, rows, seed = case
    cloud = FC.cloud_b(rows, seed)
    assert len(cloud[0]) - len(FC.kept_rows(cloud)[0]) == FC.B_DEAD
    P = FR.prepare(*cloud, res, nb, relax, np.float64)
    counts, flagged = FR.block_counts(P)
    assert flagged.mean() <= FC.FLAGGED_CAP, int(flagged.sum())
    nowhere = ~(P.inside[0].any(1) & P.inside[1].any(1) & P.inside[2].any(1))
    if relax == 0.0:
        assert (counts == 0).any() and nowhere.any()
        if res == nb:
            assert counts.sum() == 0 and nowhere.all()               # the num_refs == 0 path, with Gaussians kept
        else:
            assert counts.sum() > 0 and not nowhere.all()
    else:
        assert not nowhere.any()
        assert counts.max() > FC.constants()["CHUNK"] or nb == FC.constants()["MAX_BLOCKS"]
        # real cuts: the lists differ from block to block, and not symmetrically in x and z - a block that read another's
        # list, or a transposed decomposition, would show
        assert nb == 1 or (len(np.unique(counts)) > 1 and not np.array_equal(counts, counts.transpose(2, 1, 0)))
        assert nb <= 4 or (counts == 0).any()


@pytest.mark.parametrize("K", FC.c_lengths())
def test_c_lists_exactly_k_records_and_every_one_is_visible(K):
    cloud = FC.cloud_c(K)
    assert len(FC.kept_rows(cloud)[0]) == K and len(cloud[0]) == K + FC.C_DEAD
    for res, nb in FC.C_FORMS:
        P = FR.prepare(*cloud, res, nb, FC.all_listed(nb), np.float64)
        counts, flagged = FR.block_counts(P)
        assert (counts == K).all() and not flagged.any()
        share = FC.presence(cloud, res, nb)
        assert share.shape == (K,) and share.min() >= FC.PRESENCE, (res, nb, float(share.min()))
    # the gate cannot hide a lost record: the floor of its relative bound is far below the share of any one of them
    assert FC.gate_bounds(0.0, 1.0)[0] * 50 <= FC.PRESENCE


@pytest.mark.parametrize("rows", FC.D_CASES, ids=lambda c: "P%d-K%d" % c)
def test_d_keeps_the_same_records_scattered_and_compacted(rows):
    P_rows, K = rows
    scattered, compact, pos = FC.cloud_d(P_rows, K)
    assert len(scattered[0]) == P_rows and len(compact[0]) == K and len(pos) == K
    assert set(FC.d_pinned(P_rows)) <= set(pos.tolist()) and {0, 63, 64, 255, 256, P_rows - 1} <= set(pos.tolist())
    assert (P_rows <= 257) or 257 in pos
    for res, nb, relax in FC.D_FORMS:
        a = FR.prepare(*scattered, res, nb, relax, np.float32)
        b = FR.prepare(*compact, res, nb, relax, np.float32)
        assert np.array_equal(a.index, pos) and b.keep.all()
        assert np.array_equal(a.center, b.center) and a.scale == b.scale
        for name in ("n", "s", "q", "opacity"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert all(np.array_equal(x, y) for x, y in zip(a.inside, b.inside))
        counts, flagged = FR.block_counts(a)
        assert not flagged.any() and counts.max() > 0
        assert (counts == K).all() == (relax > 1.5)


def test_e_clouds_span_no_extent():
    clouds = FC.clouds_e()
    assert len(clouds) == 3
    for name, (cloud, point) in clouds.items():
        kept = FC.kept_rows(cloud)
        assert len(kept[0]) >= 1 and (kept[0] == point).all() and np.isfinite(point).all(), name
        with pytest.raises(ZeroDivisionError):                      # the definition divides by the extent: no reference value
            FR.prepare(*cloud, 16, 4, 1.5, np.float64)
    assert {name: (len(c[0]), len(FC.kept_rows(c)[0])) for name, (c, _) in clouds.items()} == {
        "one row": (1, 1), "one kept row among dead ones": (70, 1), "five coincident rows": (5, 5)}


def test_refused_dimensions_break_the_integer_rules_and_the_float_assertion_is_gone():
    from humangaussian_amd import fields
    c = FC.constants()
    ok = lambda res, nb: (1 <= nb <= c["MAX_BLOCKS"] and nb <= res <= c["MAX_RES"] and res % nb == 0  # noqa: E731
                          and res // nb <= c["MAX_SPLIT"])
    refused = FC.refused()
    assert not any(ok(res, nb) for res, nb in refused)
    assert {nb for _, nb in refused} >= {0, c["MAX_BLOCKS"] + 1}
    assert any(res == c["MAX_RES"] + 1 for res, _ in refused)
    assert any(nb >= 1 and res % nb == 0 and res // nb == c["MAX_SPLIT"] + 1 and res <= c["MAX_RES"] for res, nb in refused)
    assert any(nb >= 1 and res % nb != 0 for res, nb in refused)
    cpu = (torch.zeros(4, 3), torch.ones(4, 1), torch.ones(4, 3), torch.ones(4, 4))
    cloud = FC.cloud_d(257, 150)[1]
    for res, nb in FC.ACCEPTED:
        assert ok(res, nb) and res % (2 / nb) != 0                  # what the reference's assertion refused
        P = FR.prepare(*cloud, res, nb, 1.5, np.float64)            # the restatement takes it
        assert P.split * nb == res and len(P.lo) == nb
        with pytest.raises(RuntimeError, match="HIP device"):       # ... and so does the package, up to the device check
            fields.extract_fields(cpu, res, nb)
    for res, nb in refused:
        if nb < 1 or res % nb:
            with pytest.raises(ValueError):
                fields.extract_fields(cpu, res, nb)
