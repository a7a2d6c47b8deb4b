"""GPU tests of the density field and marching cubes (csrc/fields.hip through humangaussian_amd.fields): the field and
the blocks' list lengths against the fp64 restatement (tests/fields_reference.py) with the reference's own fp32 formula as
the yardstick, bit-reproducibility, the surface against the per-cell CPU marching cubes, avatar -> mesh -> MeshIndex ->
anchoring end to end, and a timing record beside a torch restatement of the reference's block loop.  The figures of the
parity and timing tests go to profiles/fields_parity.json."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_reference as FR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "fields_parity.json")


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


def _avatar(n, seed):
    """A synthetic avatar cloud: points on the humanoid of synth, anisotropic scales, random rotations."""
    from humangaussian_amd import synth
    rng = np.random.default_rng(seed)
    xyz = synth.humanoid_points(n, seed=seed).astype(np.float32)
    scaling = (0.012 * np.exp(0.5 * rng.normal(size=(n, 3)))).astype(np.float32)
    rotation = rng.normal(size=(n, 4)).astype(np.float32)
    opacity = (0.002 + 0.95 * rng.uniform(size=(n, 1))).astype(np.float32)
    return xyz, opacity, scaling, rotation


def _fixture():
    d = np.load(os.path.join(ROOT, "tests", "golden", "reference_fields.npz"))
    return d["xyz"], d["opacity"], d["scaling"], d["rotation"]


def _dense():
    return FR.cloud(6000, 5, surface=False)


def _sparse():
    """A small cluster and two far Gaussians that stretch the box: most blocks are empty."""
    rng = np.random.default_rng(11)
    xyz = np.concatenate([rng.normal(size=(500, 3)) * 0.03 + (0.1, -0.05, 0.2), [(0, 0, -1.0), (0, 0, 1.0)]]).astype(np.float32)
    n = len(xyz)
    return (xyz, np.full((n, 1), 0.7, np.float32), (0.01 * np.exp(0.4 * rng.normal(size=(n, 3)))).astype(np.float32),
            rng.normal(size=(n, 4)).astype(np.float32))


# name: (cloud, resolution, num_blocks).  The seeds were chosen so that the restatement alone flags at most 0.1 % of the
# blocks as "a Gaussian within 1e-6 of a cut plane" (checked without a GPU by tests/test_fields_cpu.py).
CASES = {"avatar": (lambda: _avatar(12000, 6), 128, 16), "fixture": (_fixture, 32, 8), "dense": (_dense, 32, 4),
         "sparse": (_sparse, 64, 16)}


def _to_dev(cloud):
    return tuple(torch.as_tensor(a, device=DEV) for a in cloud)


@pytest.mark.parametrize("case", sorted(CASES))
def test_field_against_the_fp64_restatement(case):
    from humangaussian_amd.fields import extract_fields
    make, res, nb = CASES[case]
    cloud = make()
    occ, center, scale, counts = extract_fields(_to_dev(cloud), res, nb, return_block_counts=True)
    assert occ.shape == (res,) * 3 and occ.dtype == torch.float32 and counts.shape == (nb,) * 3 and counts.dtype == torch.int32
    ref64, P = FR.field(*cloud, resolution=res, num_blocks=nb, dtype=np.float64)
    ref32, _ = FR.field(*cloud, resolution=res, num_blocks=nb, dtype=np.float32)
    # the blocks' lists: exactly the restatement's, but for blocks with a Gaussian within 1e-6 of a cut plane
    want, flagged = FR.block_counts(P)
    got = counts.cpu().numpy().astype(np.int64)
    print(f"{case}: flagged blocks {np.argwhere(flagged).tolist()}, fullest list {want.max()}, empty {int((want == 0).sum())} of {want.size}")
    assert flagged.mean() <= 1e-3, flagged.sum()
    assert np.array_equal(got[~flagged], want[~flagged]), np.argwhere((got != want) & ~flagged)[:10]
    if case == "dense":
        assert want.max() >= 4 * 256            # at least four LDS chunks in the fullest block
    if case == "sparse":
        assert (want == 0).mean() > 0.5
    # center / scale
    np.testing.assert_allclose(center.cpu().numpy(), P.center, rtol=0, atol=1e-6 * max(1.0, float(np.abs(P.center).max())))
    assert abs(scale - P.scale) <= 1e-6 * P.scale
    # values: no farther from fp64 than 1.25 x what the reference's own formula loses in fp32
    e, _ = FR.distance(ref32, ref64)
    clean = np.ones(occ.shape, bool)               # samples of flagged blocks are not comparable
    s = res // nb
    for bx, by, bz in np.argwhere(flagged & (got != want)):
        clean[bx * s:(bx + 1) * s, by * s:(by + 1) * s, bz * s:(bz + 1) * s] = False
    o = occ.cpu().numpy().astype(np.float64)
    big = (ref64 > 1e-3 * ref64.max()) & clean
    rel = float((np.abs(o - ref64)[big] / ref64[big]).max())
    small = (~(ref64 > 1e-3 * ref64.max())) & clean
    ab = float(np.abs(o - ref64)[small].max()) if small.any() else 0.0
    print(f"{case}: e = {e:.3e} (fp32 reference formula vs fp64), kernel rel {rel:.3e} abs {ab:.3e}, max {ref64.max():.4f}")
    _record("parity_" + case, {"e_fp32_reference_formula": e, "kernel_rel": rel, "kernel_abs_small": ab,
                               "field_max": float(ref64.max()), "gaussians": int(len(cloud[0])), "resolution": res,
                               "num_blocks": nb, "fullest_list": int(want.max()), "flagged_blocks": int(flagged.sum())})
    assert rel <= 1.25 * e, (rel, e)
    assert ab <= 1.25 * e * 1e-3 * ref64.max(), (ab, e)


def test_field_is_bit_reproducible():
    from humangaussian_amd.fields import extract_fields
    from humangaussian_amd.knn import distCUDA2
    cloud = _to_dev(_avatar(20000, 9))
    a = extract_fields(cloud, 64, 16)[0]
    b = extract_fields(cloud, 64, 16)[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    distCUDA2(cloud[0])                                            # unrelated work in between
    torch.randn(1 << 20, device=DEV).sum().item()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = extract_fields(cloud, 64, 16)[0]
    st.synchronize()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert a.max().item() > 0


def _sphere(shape, r):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)
    c = (np.array(shape) - 1) / 2 + np.array([0.13, -0.21, 0.07])
    return (r - np.linalg.norm(g - c, axis=-1)).astype(np.float32)


def _torus(shape, R, r):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)
    c = (np.array(shape) - 1) / 2 + np.array([0.11, 0.17, -0.05])
    d = g - c
    return (r - np.sqrt((np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) - R) ** 2 + d[..., 2] ** 2)).astype(np.float32)


def _check_surface(field, thr, chi):
    from scipy.spatial import cKDTree
    from humangaussian_amd.fields import marching_cubes
    v, t = marching_cubes(torch.as_tensor(field, device=DEV), thr)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    v, t = v.cpu().numpy(), t.cpu().numpy().astype(np.int64)
    soup = FR.marching_cubes(field, thr)
    rv, rf = FR.weld(soup, 4)
    assert len(t) == len(soup)
    assert len(v) == len(rv)
    # the same set of vertices to 1e-4 in index units
    assert cKDTree(rv).query(v)[0].max() <= 1e-4 and cKDTree(v).query(rv)[0].max() <= 1e-4
    assert t.min() >= 0 and t.max() < len(v)
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
    assert len(np.unique(t)) == len(v)                             # every vertex is used
    assert FR.is_closed(t) and FR.is_oriented(t)
    assert FR.euler(v, t) == FR.euler(rv, rf)
    if chi is not None:
        assert FR.euler(v, t) == chi
    vol = FR.signed_volume(v, t)
    assert vol > 0 and abs(vol - FR.signed_volume(rv, rf)) <= 1e-4 * vol
    return v, t


def test_marching_cubes_sphere_torus_and_non_cubic_fields():
    _check_surface(_sphere((40, 40, 40), 13.3), 0.0, 2)
    _check_surface(_torus((48, 48, 24), 13.7, 5.2), 0.0, 0)
    v, _ = _check_surface(_sphere((23, 31, 17), 6.4), 0.25, 2)     # three different sizes
    assert v[:, 0].max() <= 22 and v[:, 1].max() <= 30 and v[:, 2].max() <= 16 and v.min() >= 0


def _two_spheres(shape, boxes, centres, r=6.4):
    """-r everywhere, inside each box (lo, hi) the signed distance field of a sphere of radius r: the boxes' faces lie outside"""
    field = np.full(shape, -r, np.float32)
    for (lo, hi), c in zip(boxes, centres):
        g = np.stack(np.meshgrid(*[np.arange(a, b, dtype=np.float64) for a, b in zip(lo, hi)], indexing="ij"), -1)
        field[tuple(slice(a, b) for a, b in zip(lo, hi))] = (r - np.linalg.norm(g - np.array(c), axis=-1)).astype(np.float32)
    return field


# (field shape, the two crops, the spheres' centres).  The first field has 1,056,768 samples, i.e. 1032 scan blocks, and
# its second sphere near index (53, 117, 118) - flat index ~890k, still inside the first round of 1024 blocks: there the
# blocks behind 2^20 and the totals take the carry, no vertex does.  In the second field the second
# sphere lies entirely behind flat index 2^20 (x >= 4096 with 256 samples per x): every vertex and triangle offset of it
# is the first sphere's total, carried into the second round, plus a prefix inside that round.
TWO_SPHERES = {
    "64x128x129": ((64, 128, 129), [((0, 0, 0), (24, 24, 24)), ((42, 106, 107), (64, 128, 129))],
                   [(10.13, 9.79, 10.07), (53.13, 116.79, 118.07)]),
    "4120x16x16": ((4120, 16, 16), [((0, 0, 0), (24, 16, 16)), ((4097, 0, 0), (4120, 16, 16))],
                   [(10.13, 7.62, 7.41), (4105.13, 7.62, 7.41)]),
}


@pytest.mark.parametrize("case", sorted(TWO_SPHERES))
def test_marching_cubes_offsets_carry_past_one_round_of_the_block_scan(case):
    """More than 2^20 samples: the one-workgroup pass of the (vertices, triangles) scan (gridscan.h: hgs_scan_carry on
    uint2) runs a second round.  Two spheres; the surface of the whole field must be the surfaces of the two cropped
    sub-boxes (each at most 32^3: the single-round path test_marching_cubes_sphere_torus_and_non_cubic_fields checks), one
    behind the other: triangles are emitted in flat-index order and cropping preserves that order, so the triangle list
    equals the concatenation EXACTLY, the second crop's indices offset by the first crop's vertex count; the vertices
    agree to 1e-4 index units after the shift (the gate of _check_surface; the shift changes the rounding of x + t) - on
    the long axis of the second field to the spacing of fp32 at 4119, which is coarser than 1e-4."""
    from humangaussian_amd.fields import marching_cubes
    shape, boxes, centres = TWO_SPHERES[case]
    assert np.prod(shape) > (1 << 20) and all(max(b - a for a, b in zip(lo, hi)) <= 32 for lo, hi in boxes)
    field = _two_spheres(shape, boxes, centres)
    thr = 0.25
    v, t = marching_cubes(torch.as_tensor(field, device=DEV), thr)
    parts = [marching_cubes(torch.as_tensor(np.ascontiguousarray(field[tuple(slice(a, b) for a, b in zip(lo, hi))]), device=DEV), thr)
             for lo, hi in boxes]
    (v1, t1), (v2, t2) = parts
    assert len(v1) > 100 and len(v2) > 100 and len(t1) > 100 and len(t2) > 100
    want_t = torch.cat([t1, t2 + len(v1)])
    assert t.shape == want_t.shape and torch.equal(t, want_t)
    want_v = torch.cat([v1 + torch.tensor(boxes[0][0], dtype=torch.float32, device=DEV),
                        v2 + torch.tensor(boxes[1][0], dtype=torch.float32, device=DEV)])
    # per axis: 1e-4, or where the coordinates are so large that fp32 is coarser than that (x up to 4119: spacing 2^-11)
    # the two roundings by which the sides differ - x + t here, (x' + t) + shift there - of half a spacing each
    tol = torch.tensor([max(1e-4, float(np.spacing(np.float32(n - 1)))) for n in shape], device=DEV)
    assert v.shape == want_v.shape and ((v - want_v).abs().amax(0) <= tol).all(), (v - want_v).abs().amax(0)


def test_marching_cubes_avatar_field_at_threshold_one():
    from humangaussian_amd.fields import extract_fields
    occ = extract_fields(_to_dev(_avatar(20000, 4)), 64, 16)[0]
    f = occ.cpu().numpy()
    assert f.max() > 1 > f.min()
    _check_surface(f, 1.0, None)


def test_marching_cubes_empty_results_and_the_inside_rule():
    from humangaussian_amd.fields import marching_cubes
    for fill in (0.0, 2.0):                                        # entirely below / entirely above the threshold
        v, t = marching_cubes(torch.full((9, 8, 7), fill, device=DEV), 1.0)
        assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32
    # a field with a dimension of one sample has no cell: crossed edges there belong to no cell and give no vertex
    flat = torch.zeros(6, 5, 1, device=DEV)
    flat[2:4, 1:3, 0] = 2.0
    for shape in ((6, 5, 1), (6, 1, 5), (1, 6, 5)):
        v, t = marching_cubes(flat.reshape(shape), 1.0)
        assert v.shape == (0, 3) and t.shape == (0, 3), shape
    assert len(FR.marching_cubes(flat.cpu().numpy(), 1.0)) == 0
    # value == threshold counts as INSIDE: one sample at the threshold in a field below it is a (degenerate) closed
    # surface of six edges, all of whose vertices sit on the sample; with the sample just below there is nothing
    f = torch.zeros(5, 5, 5, device=DEV)
    f[2, 2, 2] = 1.0
    v, t = marching_cubes(f, 1.0)
    assert v.shape == (6, 3) and t.shape == (8, 3)
    assert torch.equal(v, torch.full((6, 3), 2.0, device=DEV))
    assert FR.is_closed(t.cpu().numpy())
    f[2, 2, 2] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    v, t = marching_cubes(f, 1.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)
    # a plane of samples at the threshold above higher values: inside includes the plane, the surface lies on it
    g = torch.zeros(4, 4, 6, device=DEV)
    g[:, :, :3] = 2.0
    g[:, :, 3] = 1.0
    v, t = marching_cubes(g, 1.0)
    assert len(v) == 16 and torch.equal(v[:, 2], torch.full((16,), 3.0, device=DEV)) and len(t) == 18
    n = torch.cross(v[t[:, 1].long()] - v[t[:, 0].long()], v[t[:, 2].long()] - v[t[:, 0].long()], dim=1)
    assert (n[:, 2] > 0).all()                                      # normals from high values to low


def test_extract_mesh_feeds_the_mesh_index_and_the_anchoring():
    from humangaussian_amd.animation import anchor_to_mesh
    from humangaussian_amd.fields import extract_mesh
    from humangaussian_amd.mesh import MeshIndex
    cloud = _avatar(20000, 4)
    xyz, opacity, scaling, rotation = _to_dev(cloud)
    v, f = extract_mesh((xyz, opacity, scaling, rotation), density_thresh=1, resolution=128)
    assert len(v) > 1000 and len(f) > 2000 and v.device.type == "cuda"
    grow = 3 * float(cloud[2].max())
    assert (v.min(0).values >= xyz.min(0).values - grow).all() and (v.max(0).values <= xyz.max(0).values + grow).all()
    assert FR.signed_volume(v.cpu().numpy(), f.cpu().numpy().astype(np.int64)) > 0
    idx = MeshIndex(v, f)                                           # takes the device tensors as they are
    dist = idx.signed_distance(xyz)[0]
    assert torch.isfinite(dist).all() and (dist.abs() <= grow).all()
    anchors, keep, err = anchor_to_mesh(xyz, v, f, max_error=0.01)
    assert keep.dtype == torch.bool and keep.shape == (len(xyz),) and keep.float().mean().item() > 0.9
    assert torch.isfinite(err).all()


def _torch_block_loop(xyz, opacity, scaling, rotation, resolution, num_blocks, relax_ratio=1.5):
    """The reference's extract_fields as plain torch on the device (written from the definition): the baseline."""
    block_size = 2 / num_blocks
    split = resolution // num_blocks
    mask = opacity.reshape(-1) > 0.005
    op, x, s, q = opacity.reshape(-1)[mask], xyz[mask], scaling[mask], rotation[mask]
    mn, mx = x.amin(0), x.amax(0)
    center, scale = (mn + mx) / 2, 1.8 / (mx - mn).amax().item()
    x, s = (x - center) * scale, s * scale
    q = q / q.norm(dim=1, keepdim=True)
    r, i, j, k = q.unbind(1)
    R = torch.stack([1 - 2 * (j * j + k * k), 2 * (i * j - r * k), 2 * (i * k + r * j), 2 * (i * j + r * k),
                     1 - 2 * (i * i + k * k), 2 * (j * k - r * i), 2 * (i * k - r * j), 2 * (j * k + r * i),
                     1 - 2 * (i * i + j * j)], 1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    S = L @ L.transpose(1, 2)
    a, b, c, d, e, f = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    inv_det = 1 / (a * d * f + 2 * e * c * b - e ** 2 * a - c ** 2 * d - b ** 2 * f + 1e-24)
    co = torch.stack([(d * f - e ** 2) * inv_det, (e * c - b * f) * inv_det, (e * b - c * d) * inv_det,
                      (a * f - c ** 2) * inv_det, (b * c - e * a) * inv_det, (a * d - b ** 2) * inv_det], 1)
    occ = torch.zeros([resolution] * 3, dtype=torch.float32, device=xyz.device)
    ax = torch.linspace(-1, 1, resolution).to(xyz.device).split(split)
    for xi, xs in enumerate(ax):
        for yi, ys in enumerate(ax):
            for zi, zs in enumerate(ax):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
                vmin, vmax = pts.amin(0) - block_size * relax_ratio, pts.amax(0) + block_size * relax_ratio
                m = (x < vmax).all(-1) & (x > vmin).all(-1)
                if not m.any():
                    continue
                mx_, mc, mo = x[m], co[m], op[m]
                val = 0
                for g0 in range(0, len(mx_), 1024):
                    dd = pts[:, None, :] - mx_[None, g0:g0 + 1024]
                    cc = mc[None, g0:g0 + 1024]
                    dx, dy, dz = dd.unbind(-1)
                    power = (-0.5 * (dx ** 2 * cc[..., 0] + dy ** 2 * cc[..., 3] + dz ** 2 * cc[..., 5]) - dx * dy * cc[..., 1]
                             - dx * dz * cc[..., 2] - dy * dz * cc[..., 4])
                    power[power > 0] = -1e10
                    val = val + (mo[None, g0:g0 + 1024] * torch.exp(power)).sum(-1)
                occ[xi * split:(xi + 1) * split, yi * split:(yi + 1) * split, zi * split:(zi + 1) * split] = val.reshape(split, split, split)
    return occ


def _event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def test_time_record_beside_the_torch_block_loop():
    """A record, not a gate beyond "the kernels are not slower than the loop": 100k Gaussians, 128^3."""
    from humangaussian_amd.fields import extract_fields, marching_cubes
    cloud = _to_dev(_avatar(100000, 1))
    occ = extract_fields(cloud, 128, 16)[0]
    loop = _torch_block_loop(*cloud, 128, 16)
    scale = loop.max().item()
    err = (occ - loop).abs().max().item()
    assert err <= 2e-3 * scale, (err, scale)                        # two fp32 evaluations of one field (sanity, not parity)
    t_field = _event_ms(lambda: extract_fields(cloud, 128, 16), 2, 7)
    t_mc = _event_ms(lambda: marching_cubes(occ, 1.0), 2, 7)
    t_loop = _event_ms(lambda: _torch_block_loop(*cloud, 128, 16), 1, 2)
    v, t = marching_cubes(occ, 1.0)
    print(f"extract_fields {t_field:.3f} ms, marching_cubes {t_mc:.3f} ms ({len(v)} vertices, {len(t)} triangles), "
          f"torch block loop {t_loop:.1f} ms")
    _record("time_100k_128", {"extract_fields_ms": t_field, "marching_cubes_ms": t_mc, "torch_block_loop_ms": t_loop,
                              "vertices": int(len(v)), "triangles": int(len(t)), "max_abs_diff_vs_loop": err,
                              "field_max": scale})
    assert t_field <= t_loop
