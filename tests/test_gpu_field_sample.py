"""GPU tests of the field's point samples (csrc/fields.hip: hgs_k_fsample_*, through humangaussian_amd.fields.GaussianField):
density, normal and colour against the fp64 restatement (tests/field_sample_reference.py) with the same formulas in fp32 as
the yardstick, the field's own bits at the grid samples, every list length and bin size around the staging chunk and the
run of 256 points, membership at and beyond the block planes, bit-reproducibility under permutation, and the coloured,
shaded mesh end to end.  The measured ratios go to profiles/field_sample_parity.json."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_sample_cases as C  # noqa: E402
import field_sample_reference as SR  # noqa: E402
import fields_cases as FC  # noqa: E402
import fields_reference as FR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "field_sample_parity.json")
MARGIN = 4.0          # both sides are the same formulas in fp32: their maxima over a few thousand points differ by rounding luck


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


def _field(cloud, res, nb, relax=1.5):
    from humangaussian_amd.fields import GaussianField
    return GaussianField(_to_dev(cloud), res, nb, relax)


def _sample(field, pts, colors=None, normalized=False):
    d, n, c = field.sample(torch.as_tensor(np.ascontiguousarray(pts), device=DEV),
                           None if colors is None else torch.as_tensor(colors, device=DEV), normalized)
    assert d.dtype == torch.float32 and d.shape == (len(pts),) and n.dtype == torch.float32 and n.shape == (len(pts), 3)
    assert (c is None) == (colors is None) and (c is None or (c.dtype == torch.float32 and c.shape == (len(pts), 3)))
    return d.cpu().numpy(), n.cpu().numpy(), None if c is None else c.cpu().numpy()


def _bits(got):
    return tuple(None if a is None else np.ascontiguousarray(a).view(np.int32) for a in got)


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _gate(name, got, ref64, ref32, keep, record=None):
    """The kernel's outputs over the points `keep` no farther from fp64 than MARGIN x what the restatement loses in fp32."""
    assert keep.sum() > 0
    r64 = SR.subset(ref64, keep)
    r32 = SR.subset(ref32, keep)
    e = SR.errors((r32.density, r32.normal, r32.color), r64)
    k = SR.errors(tuple(None if a is None else a[keep] for a in got), r64)
    top = float(r64.density.max())
    fmt = lambda t: ", ".join("none" if v is None else f"{v:.3e}" for v in t)  # noqa: E731
    print(f"{name}: {int(keep.sum())} points, density max {top:.4f}; (density rel, density abs below the floor, colour abs, "
          f"normal angle) restatement in fp32: {fmt(e)}; kernel: {fmt(k)}")
    if record:
        ratio = lambda a, b: None if a is None else (a / b if b > 0 else (0.0 if a == 0 else float("inf")))  # noqa: E731
        _record(record, {"points": int(keep.sum()), "density_max": top, "e_density_rel": e[0], "e_color_abs": e[2],
                         "e_normal_angle": e[3], "kernel_density_rel": k[0], "kernel_density_abs_small": k[1],
                         "kernel_color_abs": k[2], "kernel_normal_angle": k[3], "ratio_density": ratio(k[0], e[0]),
                         "ratio_color": ratio(k[2], e[2]), "ratio_normal": ratio(k[3], e[3])})
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and (got[2] is None or np.isfinite(got[2]).all())
    assert k[0] <= MARGIN * e[0], ("density", k[0], e[0])
    assert k[1] <= MARGIN * e[0] * 1e-3 * top, ("density below the floor", k[1], e[0], top)
    if k[2] is not None:
        assert k[2] <= MARGIN * e[2], ("colour", k[2], e[2])
    assert k[3] <= MARGIN * e[3], ("normal", k[3], e[3])


def _clean_blocks(field, P):
    """(nb,)*3 bool: blocks whose list is the restatement's.  The lists must agree everywhere but in blocks that hold a
    Gaussian within 1e-6 of a cut plane (tests/test_gpu_fields.py holds the kernel to the same)."""
    want, flagged = FR.block_counts(P)
    got = field.block_counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(got[~flagged], want[~flagged])
    return ~(flagged & (got != want)), want


# ------------------------------------------------------------------------------------------------ parity on three clouds

@pytest.mark.parametrize("form", ["normalised", "world"])
@pytest.mark.parametrize("case", C.CASES)
def test_samples_against_the_fp64_restatement(case, form):
    """The mesh's own vertices and 2 000 uniform points of the box grown by 10 %.  Normalised coordinates: every point is
    compared (membership is exact).  World coordinates: points within 1e-6 of a plane between two blocks are not - at most
    0.1 % of the uniform points, and the share of the vertices that lie on such planes by construction (two of a
    marching-cubes vertex's coordinates are grid samples; tests/test_field_sample_cpu.py)."""
    from humangaussian_amd.fields import marching_cubes
    cloud, res, nb = C.cloud_of(case)
    field = _field(cloud, res, nb)
    v, _ = marching_cubes(field.occ, C.threshold(field.occ.max().item()))
    vn = v / (res - 1.0) * 2 - 1                                      # as extract_mesh has them
    assert len(vn) >= 50
    uni = C.uniform_points(case)
    pts = torch.cat([vn, torch.as_tensor(uni, device=DEV)])
    normalized = form == "normalised"
    if not normalized:
        pts = pts / field.scale + field.center
    pts = pts.cpu().numpy()
    colors = C.colors_of(len(cloud[0]))
    got = _sample(field, pts, colors, normalized)
    ref64 = SR.sample(cloud, pts, colors, res, nb, dtype=np.float64, normalized=normalized)
    ref32 = SR.sample(cloud, pts, colors, res, nb, dtype=np.float32, normalized=normalized)
    clean, want = _clean_blocks(field, ref64.prepared)
    keep = clean[ref64.block[:, 0], ref64.block[:, 1], ref64.block[:, 2]] & ref64.finite
    if not normalized:
        assert ref64.near[len(vn):].mean() <= C.NEAR_CAP
        keep &= ~ref64.near
        print(f"{case}: {int(ref64.near[:len(vn)].sum())} of {len(vn)} vertices on a plane between two blocks are not compared")
    else:
        assert np.array_equal(ref32.block, ref64.block)
    assert keep[:len(vn)].sum() >= 40 and keep[len(vn):].mean() >= 0.99
    if case == "dense":
        assert want.max() >= 4 * 256
    if case == "sparse":
        assert (want == 0).mean() > 0.5
    _gate(f"{case} {form}", got, ref64, ref32, keep, record=f"parity_{case}_{form}")


# ------------------------------------------------------------------------------------------------ the field's own bits

def test_grid_samples_return_occ_bit_for_bit():
    cloud, res, nb = C.cloud_of("fixture")
    field = _field(cloud, res, nb)
    ax = torch.linspace(-1, 1, res).to(DEV)
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    d, n, c = field.sample(pts, None, normalized=True)
    assert c is None and field.occ.max().item() > 0
    assert torch.equal(d.view(torch.int32), field.occ.reshape(-1).view(torch.int32))
    from humangaussian_amd.fields import extract_fields
    occ = extract_fields(_to_dev(cloud), res, nb)[0]                     # ... which are extract_fields' bits
    assert torch.equal(occ.view(torch.int32), field.occ.view(torch.int32))
    norm = n.norm(dim=1)
    assert (((norm - 1).abs() <= 1e-6) | (norm == 0)).all()


# ------------------------------------------------------------------------------------------------ list lengths

LIST_FORM = (8, 2)          # resolution, num_blocks; with fields_cases.all_listed every block lists every kept Gaussian


@pytest.mark.parametrize("K", [1, 255, 256, 257, 512, 513])
def test_every_list_length_around_the_staging_chunk(K):
    """Exactly K kept Gaussians among dead rows, every block listing all of them: one record, and both sides of one and of
    two staging chunks.  (K = 1: one kept Gaussian spans no extent, the plan lists nothing - the field's contract - and
    every sample is zero; a list of ONE record is held to the gate by the two-Gaussian cloud below.)"""
    assert FC.constants()["CHUNK"] == 256
    res, nb = LIST_FORM
    cloud = FC.cloud_c(K) if K > 1 else FC.scatter(FC.wide(1, 501), 1 + FC.C_DEAD, 701)[0]
    assert int(((cloud[1].reshape(-1) > FR.OPACITY_CUT) & np.isfinite(cloud[0]).all(1)).sum()) == K
    field = _field(cloud, res, nb, FC.all_listed(nb))
    pts = np.random.default_rng(K).uniform(-1.1, 1.1, size=(1500, 3)).astype(np.float32)
    colors = C.colors_of(len(cloud[0]), seed=K)
    got = _sample(field, pts, colors, True)
    if K == 1:
        assert (field.block_counts == 0).all()
        assert all((a == 0).all() for a in got)
        return
    assert (field.block_counts == K).all()
    ref64 = SR.sample(cloud, pts, colors, res, nb, FC.all_listed(nb), dtype=np.float64, normalized=True)
    ref32 = SR.sample(cloud, pts, colors, res, nb, FC.all_listed(nb), dtype=np.float32, normalized=True)
    _gate(f"K = {K}", got, ref64, ref32, np.ones(len(pts), bool), record=f"list_length_{K}")


def test_lists_of_one_record():
    """Two Gaussians in opposite corners and a growth that keeps each out of the other's blocks: lists of 0 and 1."""
    xyz = np.array([(-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)], np.float32)
    cloud = (xyz, np.array([[0.8], [0.6]], np.float32), np.array([(0.1, 0.2, 0.15), (0.2, 0.1, 0.12)], np.float32),
             np.array([(1, 0.2, 0.1, 0), (0.3, 1, 0, 0.5)], np.float32))
    res, nb, relax = 8, 2, 0.25
    field = _field(cloud, res, nb, relax)
    counts = field.block_counts.cpu().numpy()
    assert counts[0, 0, 0] == 1 and counts[1, 1, 1] == 1 and counts.sum() == 2
    pts = np.random.default_rng(9).uniform(-1.1, 1.1, size=(1200, 3)).astype(np.float32)
    colors = np.array([(0.2, 0.9, 0.4), (0.7, 0.1, 0.3)], np.float32)
    got = _sample(field, pts, colors, True)
    ref64 = SR.sample(cloud, pts, colors, res, nb, relax, dtype=np.float64, normalized=True)
    ref32 = SR.sample(cloud, pts, colors, res, nb, relax, dtype=np.float32, normalized=True)
    _gate("lists of one", got, ref64, ref32, np.ones(len(pts), bool))
    own = (ref64.block == 0).all(1) | (ref64.block == 1).all(1)
    assert all((a[~own] == 0).all() for a in got)                       # blocks that receive points and list nothing
    assert (got[0][own] > 0).any()


# ------------------------------------------------------------------------------------------------ points per block

CUT = ("fixture", 32, 8, 0.0)       # relax_ratio 0: the lists of neighbouring blocks are disjoint, membership decides everything


def _cut_field():
    cloud = C.cloud_of(CUT[0])[0]
    return cloud, _field(cloud, CUT[1], CUT[2], CUT[3])


def _points_in_block(rng, ax, split, block, n):
    """n points strictly inside the block's cells (normalised coordinates)."""
    lo = np.array([ax[b * split] for b in block], np.float64)
    hi = np.array([ax[b * split + split] if b * split + split < len(ax) else ax[-1] + (ax[1] - ax[0]) for b in block], np.float64)
    return (lo + (hi - lo) * rng.uniform(0.05, 0.95, size=(n, 3))).astype(np.float32)


def test_every_bin_size_around_the_run_of_256_points():
    """Exactly 0, 1, 255, 256 and 257 points in one block with the rest spread over the others, and all points in one block:
    a point's outputs do not depend on how many points share its bin, nor on where it stands - every arrangement returns
    the bits of one base call (itself held to the fp64 gate)."""
    cloud, field = _cut_field()
    res, nb = CUT[1], CUT[2]
    split = res // nb
    ax = FR.axis_samples(res)
    counts = field.block_counts.cpu().numpy()
    target = tuple(int(i) for i in np.unravel_index(counts.argmax(), counts.shape))
    assert counts[target] > 0 and (counts == 0).any()
    rng = np.random.default_rng(12)
    inside = _points_in_block(rng, ax, split, target, 600)
    others = rng.uniform(-1.1, 1.1, size=(3000, 3)).astype(np.float32)
    blk = np.stack([SR.cells(ax, others[:, a]) for a in range(3)], 1) // split
    others = others[~(blk == np.array(target)).all(1)][:1500]
    pool = np.concatenate([inside, others])
    colors = C.colors_of(len(cloud[0]))
    base = _sample(field, pool, colors, True)
    ref64 = SR.sample(cloud, pool, colors, res, nb, CUT[3], dtype=np.float64, normalized=True)
    ref32 = SR.sample(cloud, pool, colors, res, nb, CUT[3], dtype=np.float32, normalized=True)
    assert (ref64.block[:600] == np.array(target)).all() and not (ref64.block[600:] == np.array(target)).all(1).any()
    clean, want = _clean_blocks(field, ref64.prepared)
    _gate("bins", base, ref64, ref32, clean[ref64.block[:, 0], ref64.block[:, 1], ref64.block[:, 2]])
    empty = want[ref64.block[:, 0], ref64.block[:, 1], ref64.block[:, 2]] == 0
    assert empty.sum() > 10 and all((a[empty] == 0).all() for a in base)           # points in blocks that list nothing
    for k in (0, 1, 255, 256, 257, 600):
        for rest in ((True, False) if k else (True,)):
            pick = np.concatenate([np.arange(k), np.arange(600, len(pool)) if rest else np.zeros(0, np.int64)]).astype(np.int64)
            pick = rng.permutation(pick)
            got = _sample(field, pool[pick], colors, True)
            assert _same_bits(got, tuple(a[pick] for a in base)), (k, rest)


def test_membership_at_the_block_planes_and_beyond_the_grid():
    cloud, field = _cut_field()
    res, nb = CUT[1], CUT[2]
    split = res // nb
    ax = FR.axis_samples(res)
    rng = np.random.default_rng(13)
    P32 = FR.prepare(*cloud, res, nb, CUT[3], np.float32)
    near_cloud = lambda n: (P32.n[rng.integers(0, len(P32.n), n)] + rng.normal(size=(n, 3)) * 0.03).astype(np.float32)  # noqa: E731
    on, below = [], []
    for b in range(1, nb):                                               # the first sample of block b on one axis, the other two near the cloud
        for a in range(3):
            p = near_cloud(40)
            p[:, a] = ax[b * split]
            on.append(p)
            q = p.copy()
            q[:, a] = np.nextafter(ax[b * split], np.float32(-2))
            below.append(q)
    far = near_cloud(600)
    a = np.abs(P32.n).max(0).argmax()                                    # the axis on which the cloud reaches the edge blocks
    far[:, a] = rng.choice(np.array([-1e30, -50, -1.0001, 1.0001, 3, 1e30], np.float32), 600)
    far[300:, (a + 1) % 3] = rng.choice(np.array([-7, 1.5], np.float32), 300)
    pts = np.concatenate(on + below + [far])
    colors = C.colors_of(len(cloud[0]))
    got = _sample(field, pts, colors, True)
    ref64 = SR.sample(cloud, pts, colors, res, nb, CUT[3], dtype=np.float64, normalized=True)
    ref32 = SR.sample(cloud, pts, colors, res, nb, CUT[3], dtype=np.float32, normalized=True)
    n_on = sum(len(p) for p in on)
    assert ref64.near[:2 * n_on].all() and (ref64.block[:n_on] != ref64.block[n_on:2 * n_on]).any(1).all()
    assert ((ref64.block[2 * n_on:] == 0) | (ref64.block[2 * n_on:] == nb - 1)).any(1).all()
    clean, _ = _clean_blocks(field, ref64.prepared)
    keep = clean[ref64.block[:, 0], ref64.block[:, 1], ref64.block[:, 2]]
    # the two sides of a plane sum disjoint lists: a point given to the wrong block shows at the scale of the field
    _gate("planes and beyond", got, ref64, ref32, keep)
    assert (got[0][:2 * n_on] > 1e-3 * ref64.density.max()).sum() > 100 and (got[0][2 * n_on:] > 0).sum() > 10


def test_points_that_are_not_finite_empty_inputs_and_empty_plans():
    from humangaussian_amd.fields import GaussianField
    cloud, res, nb = C.cloud_of("fixture")
    field = _field(cloud, res, nb)
    colors = C.colors_of(len(cloud[0]))
    pts = np.random.default_rng(14).uniform(-0.3, 0.3, size=(700, 3)).astype(np.float32)
    bad = np.arange(0, 700, 7)
    pts_bad = pts.copy()
    pts_bad[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[(bad // 7) % 3]
    for normalized in (True, False):
        good = _sample(field, pts, colors, normalized)
        got = _sample(field, pts_bad, colors, normalized)
        assert all((a[bad] == 0).all() for a in got)
        rest = np.setdiff1d(np.arange(700), bad)
        assert _same_bits(tuple(a[rest] for a in got), tuple(a[rest] for a in good)) and (good[0] > 0).any()
    # a world coordinate that overflows in the normalisation
    huge = np.full((3, 3), 3e38, np.float32)
    assert all((a == 0).all() for a in _sample(field, huge, colors, False))
    # M == 0
    d, n, c = _sample(field, np.zeros((0, 3), np.float32), colors, False)
    assert d.shape == (0,) and n.shape == (0, 3) and c.shape == (0, 3)
    assert _sample(field, np.zeros((0, 3), np.float32))[2] is None
    # colours are optional, and leave density and normal as they are
    assert _same_bits(_sample(field, pts)[:2], _sample(field, pts, colors)[:2])
    with pytest.raises(ValueError, match="one row per Gaussian"):
        field.sample(torch.zeros(4, 3, device=DEV), torch.zeros(len(cloud[0]) + 1, 3, device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        field.sample(torch.zeros(4, 3))
    # a plan that keeps no Gaussian, and no Gaussian at all
    dead = tuple(a.copy() for a in cloud)
    dead[1][:] = 0.001
    for cl in (dead, tuple(a[:0] for a in cloud)):
        f = GaussianField(_to_dev(cl), res, nb)
        assert (f.occ == 0).all() and f.occ.shape == (res,) * 3 and (f.block_counts == 0).all() and f.scale == 1.0
        got = _sample(f, pts_bad, colors[:len(cl[0])], False)
        assert all((a == 0).all() for a in got)


# ------------------------------------------------------------------------------------------------ reproducibility

def test_samples_are_bit_reproducible_and_follow_a_permutation():
    cloud, res, nb = C.cloud_of("dense")
    field = _field(cloud, res, nb)
    rng = np.random.default_rng(15)
    pts = rng.uniform(-1.05, 1.05, size=(5000, 3)).astype(np.float32)
    colors = C.colors_of(len(cloud[0]))
    for normalized in (True, False):
        p = pts if normalized else C.to_world(pts, field.center.cpu().numpy(), field.scale)
        a = _sample(field, p, colors, normalized)
        torch.randn(1 << 20, device=DEV).sum().item()                    # unrelated work in between
        b = _sample(field, p, colors, normalized)
        assert _same_bits(a, b) and (a[0] > 0).sum() > 1000
        perm = rng.permutation(len(p))
        c = _sample(field, p[perm], colors, normalized)
        assert _same_bits(c, tuple(x[perm] for x in a))
    other = _field(cloud, res, nb)                                       # a second field of the same cloud
    assert _same_bits(_sample(other, pts, colors, True), _sample(field, pts, colors, True))


# ------------------------------------------------------------------------------------------------ the mesh

def test_mesh_with_normals_and_colours_end_to_end(tmp_path):
    from humangaussian_amd.fields import extract_mesh, extract_mesh_attributes, gaussian_colors
    from humangaussian_amd.ply_io import save_mesh_ply
    cloud, res = C.ellipsoid_cloud(), C.ELLIPSOID["resolution"]
    dev = _to_dev(cloud)
    colors = C.two_colours(cloud)
    v0, f0 = extract_mesh(dev, 1, res)
    v, f, n, c = extract_mesh_attributes(dev, 1, res, colors=torch.as_tensor(colors, device=DEV))
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape == v0.shape and f.shape == f0.shape
    assert torch.equal(v.view(torch.int32), v0.view(torch.int32)) and torch.equal(f, f0) and len(f) > 500
    assert n.shape == v.shape and c.shape == v.shape and n.dtype == torch.float32 and c.dtype == torch.float32
    assert extract_mesh_attributes(dev, 1, res)[3] is None                      # the four-tensor form has no colours of its own
    norm = n.norm(dim=1).cpu().numpy()
    assert (((np.abs(norm - 1) <= 1e-6) | (norm == 0))).all() and (norm > 0).mean() > 0.99
    vv, ff, nn, cc = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy(), c.cpu().numpy()
    share = SR.face_agreement(vv, ff, nn)
    print(f"ellipsoid: {len(vv)} vertices, {len(ff)} faces, {share:.4f} agree with their vertex normals")
    assert share >= 0.99
    far = C.far_from_seam(vv, cloud)
    assert (far != 0).sum() >= 0.3 * len(vv) and (far > 0).any() and (far < 0).any()
    err = np.abs(cc - np.where((far > 0)[:, None], C.RED, C.BLUE))[far != 0].max()
    print(f"two colours: {(far != 0).sum()} of {len(vv)} vertices beyond three standard deviations, largest error {err:.2e}")
    assert err <= 0.05
    assert cc.min() >= 0 and cc.max() <= 1 + 1e-6
    path = str(tmp_path / "avatar_mesh.ply")
    save_mesh_ply(path, v, f, n, c)
    rv, rf, names = C.read_mesh_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([rv["x"], rv["y"], rv["z"]], 1), vv) and np.array_equal(rf, ff)
    assert np.array_equal(np.stack([rv["nx"], rv["ny"], rv["nz"]], 1), nn)
    assert np.array_equal(np.stack([rv["red"], rv["green"], rv["blue"]], 1), np.rint(np.clip(cc, 0, 1) * 255).astype(np.uint8))

    # a model: its degree-0 colours are baked, and center / scale are set as extract_mesh sets them
    class Model:
        get_xyz, get_opacity, get_scaling, _rotation = dev
        _features_dc = ((torch.as_tensor(colors, device=DEV) - 0.5) / 0.28209479177387814).reshape(-1, 1, 3)

    model = Model()
    assert (gaussian_colors(model) - torch.as_tensor(colors, device=DEV)).abs().max().item() <= 1e-6
    vm, fm, nm, cm = extract_mesh_attributes(model, 1, res)
    assert torch.equal(vm, v) and torch.equal(fm, f) and torch.equal(nm.view(torch.int32), n.view(torch.int32))
    assert (cm - c).abs().max().item() <= 1e-5 and isinstance(model.scale, float) and model.center.shape == (3,)
