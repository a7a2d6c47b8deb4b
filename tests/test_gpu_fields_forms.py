"""GPU sweep of the density field (csrc/fields.hip through humangaussian_amd.fields.extract_fields) over every launch form of
hgs_k_field_eval and every kind of block count and list length; the table, its clouds and the gate are tests/fields_cases.py,
held to their claims without a GPU by tests/test_fields_forms_cpu.py.

  (a) all-listed: at one resolution every num_blocks gives the bits of the pinned split s = 8 (and that one passes the fp64 gate)
  (b) cut lists in every form against the fp64 restatement, relax_ratio 1.5 and 0
  (c) lists of K records, K on both sides of one and of two staging chunks, in both thread forms
  (d) dead rows change no bit
  (e) a cloud without extent: a zero field, nothing listed, no NaN
  (f) refused dimensions

The figures of every gated case go to profiles/fields_forms_parity.json."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_cases as FC  # noqa: E402
import fields_reference as FR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "fields_forms_parity.json")


def _record(key, value):
    data = {}
    if os.path.exists(PARITY_JSON):
        try:
            data = json.load(open(PARITY_JSON))
        except ValueError:
            data = {}
    data[key] = value
    os.makedirs(os.path.dirname(PARITY_JSON), exist_ok=True)
    with open(PARITY_JSON, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def _to_dev(cloud):
    return tuple(torch.as_tensor(a, device=DEV) for a in cloud)


def _extract(cloud, res, nb, relax):
    from humangaussian_amd.fields import extract_fields
    occ, center, scale, counts = extract_fields(_to_dev(cloud), res, nb, relax, return_block_counts=True)
    assert occ.shape == (res,) * 3 and occ.dtype == torch.float32 and counts.shape == (nb,) * 3 and counts.dtype == torch.int32
    return occ, center.cpu().numpy(), scale, counts.cpu().numpy().astype(np.int64)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gate(key, cloud, res, nb, relax, occ, center, scale, got):
    """The assertions of test_gpu_fields.test_field_against_the_fp64_restatement with the bounds of FC.gate_bounds."""
    ref64, ref32, P = FC.reference(key, cloud, res, nb, relax)
    want, flagged = FR.block_counts(P)
    assert flagged.mean() <= FC.FLAGGED_CAP, flagged.sum()
    assert np.array_equal(got[~flagged], want[~flagged]), np.argwhere((got != want) & ~flagged)[:10]
    np.testing.assert_allclose(center, P.center, rtol=0, atol=1e-6 * max(1.0, float(np.abs(P.center).max())))
    assert abs(scale - P.scale) <= 1e-6 * P.scale
    e, _ = FR.distance(ref32, ref64)
    clean = np.ones(ref64.shape, bool)                 # samples of flagged blocks are not comparable
    s = res // nb
    for bx, by, bz in np.argwhere(flagged & (got != want)):
        clean[bx * s:(bx + 1) * s, by * s:(by + 1) * s, bz * s:(bz + 1) * s] = False
    o = occ.cpu().numpy()
    assert np.isfinite(o).all()
    rel, ab = FC.kernel_distance(o, ref64, clean)
    bound_rel, bound_abs = FC.gate_bounds(e, float(ref64.max()))
    items, threads, slabs, odd = FC.eval_form(s)
    print(f"{key}: s = {s} ({items} items, {threads} threads, {slabs} slabs), e = {e:.3e}, kernel rel {rel:.3e} abs {ab:.3e}, "
          f"bounds {bound_rel:.3e} {bound_abs:.3e}, max {ref64.max():.4f}, fullest list {want.max()}, flagged {int(flagged.sum())}")
    _record(key, {"e_fp32_reference_formula": e, "kernel_rel": rel, "kernel_abs_small": ab, "field_max": float(ref64.max()),
                  "rows": int(len(cloud[0])), "kept": int(len(P.n)), "resolution": res, "num_blocks": nb, "split": s,
                  "relax_ratio": relax, "threads": threads, "slabs": slabs, "fullest_list": int(want.max()),
                  "flagged_blocks": int(flagged.sum())})
    assert rel <= bound_rel, (rel, e)
    assert ab <= bound_abs, (ab, e)
    return want


# ------------------------------------------------------------------------------------------------ (a)

@pytest.mark.parametrize("res", sorted(FC.A_TABLE))
def test_every_split_gives_the_bits_of_the_pinned_split(res):
    """All-listed, a sample's value depends on its position, the records and the order of the sum alone - none of which
    depends on num_blocks.  Any difference between two forms is a sample evaluated at the wrong place, twice or not at all."""
    cloud = FC.cloud_a()
    kept = len(FC.kept_rows(cloud)[0])
    nb0 = res // FC.A_PINNED_SPLIT
    assert nb0 in FC.A_TABLE[res]
    occ0, center0, scale0, counts0 = _extract(cloud, res, nb0, FC.all_listed(nb0))
    assert occ0.max().item() > 0
    if res == FC.A_GATED_RES:
        _gate(f"a_R{res}_nb{nb0}", cloud, res, nb0, FC.all_listed(nb0), occ0, center0, scale0, counts0)
    for nb in FC.A_TABLE[res]:
        occ, center, scale, counts = _extract(cloud, res, nb, FC.all_listed(nb))
        assert (counts == kept).all(), (nb, np.unique(counts))
        assert np.array_equal(center, center0) and scale == scale0, nb
        same = _bits(occ) == _bits(occ0)
        assert bool(same.all()), (res, nb, res // nb, FC.eval_form(res // nb), int((~same).sum()),
                                  (~same).nonzero()[:8].tolist())


# ------------------------------------------------------------------------------------------------ (b)

@pytest.mark.parametrize("case", FC.B_CASES, ids=FC.b_id)
def test_cut_lists_in_every_form_against_the_fp64_restatement(case):
    res, nb, relax, rows, seed = case
    cloud = FC.cloud_b(rows, seed)
    occ, center, scale, counts = _extract(cloud, res, nb, relax)
    want = _gate("b_" + FC.b_id(case), cloud, res, nb, relax, occ, center, scale, counts)
    if relax == 0.0 and res == nb:               # a block is one point: nothing is listed, the field is exactly zero
        assert want.max() == 0 and counts.max() == 0 and not occ.any().item()


# ------------------------------------------------------------------------------------------------ (c)

@pytest.mark.parametrize("K", FC.c_lengths())
@pytest.mark.parametrize("form", FC.C_FORMS, ids=lambda f: "R%d-nb%d" % f)
def test_list_lengths_on_the_staging_chunk(form, K):
    res, nb = form
    cloud = FC.cloud_c(K)
    occ, center, scale, counts = _extract(cloud, res, nb, FC.all_listed(nb))
    assert (counts == K).all(), np.unique(counts)
    _gate(f"c_R{res}_nb{nb}_K{K}", cloud, res, nb, FC.all_listed(nb), occ, center, scale, counts)


# ------------------------------------------------------------------------------------------------ (d)

@pytest.mark.parametrize("form", FC.D_FORMS, ids=lambda f: "R%d-nb%d-relax%g" % f)
@pytest.mark.parametrize("rows", FC.D_CASES, ids=lambda c: "P%d-K%d" % c)
def test_dead_rows_change_no_bit(rows, form):
    """The ballot-and-rank compaction of hgs_k_field_lists at its 64- and 256-row strides; non-finite rows stay out of the box."""
    res, nb, relax = form
    scattered, compact, pos = FC.cloud_d(*rows)
    a = _extract(scattered, res, nb, relax)
    b = _extract(compact, res, nb, relax)
    assert a[0].max().item() > 0 and b[3].max() > 0
    assert np.array_equal(a[3], b[3])
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert torch.equal(_bits(a[0]), _bits(b[0]))


# ------------------------------------------------------------------------------------------------ (e)

@pytest.mark.parametrize("name", sorted(FC.clouds_e()))
def test_a_cloud_without_extent_gives_a_zero_field(name):
    from humangaussian_amd.fields import extract_mesh
    cloud, point = FC.clouds_e()[name]
    for res, nb in ((16, 4), (9, 9), (10, 1)):
        occ, center, scale, counts = _extract(cloud, res, nb, 1.5)
        assert torch.isfinite(occ).all().item() and not occ.any().item()
        assert not counts.any()
        assert np.array_equal(center, point)
        assert scale == float("inf")
    v, f = extract_mesh(_to_dev(cloud), density_thresh=1, resolution=32)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32


# ------------------------------------------------------------------------------------------------ (f)

def test_refused_dimensions_raise_and_integer_multiples_do_not():
    from humangaussian_amd.fields import extract_fields
    cloud = FC.cloud_d(257, 150)[1]
    dev = _to_dev(cloud)
    for res, nb in FC.refused():
        with pytest.raises((ValueError, RuntimeError)):
            extract_fields(dev, res, nb)
    with pytest.raises(ValueError, match="multiple of num_blocks"):
        extract_fields(dev, 100, 16)
    # resolution % (2 / num_blocks) != 0 in floating point: accepted, and (all-listed) the bits of one block
    for res, nb in FC.ACCEPTED:
        assert res % (2 / nb) != 0 and res % nb == 0
        occ, _, _, counts = _extract(cloud, res, nb, FC.all_listed(nb))
        one = _extract(cloud, res, 1, FC.all_listed(1))[0]
        assert (counts == len(cloud[0])).all() and occ.max().item() > 0
        assert torch.equal(_bits(occ), _bits(one)), (res, nb)
