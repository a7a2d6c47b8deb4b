"""GPU tests of the mesh cleaning and decimation (csrc/meshclean.hip through humangaussian_amd.meshclean and
fields.extract_clean_mesh): components, the keep rule and the vertex clustering against the numpy restatement
(tests/mesh_clean_reference.py) BIT FOR BIT, the properties of a decimated mesh, order independence, and the public path
on an avatar with a floater."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_cases as FC  # noqa: E402
import mesh_clean_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(v, f, index=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(v, np.float32), device=DEV), torch.as_tensor(np.ascontiguousarray(f), device=DEV).to(index)


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(got, want):
    got, want = _np(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    assert np.array_equal(got, want)


def _check_components(v, f):
    from humangaussian_amd.meshclean import mesh_components
    labels, comp_faces, comp_diag2, rounds = mesh_components(*_dev(v, f), return_rounds=True)
    want = ref.components_bfs(v.shape[0], f)
    want_faces, want_diag2 = ref.component_stats(v, f, want)
    _same_bits(labels, want)
    _same_bits(comp_faces, want_faces)
    _same_bits(comp_diag2, want_diag2)
    return rounds


def _check_clean(v, f, min_f, min_d):
    from humangaussian_amd.meshclean import clean_mesh
    tv, tf = _dev(v, f)
    cv, cf, src = clean_mesh(tv, tf, min_f=min_f, min_d=min_d, return_index=True)
    wv, wf, wsrc = ref.clean(v, f, min_f, min_d)
    _same_bits(cv, wv)
    _same_bits(cf, wf)
    _same_bits(src, wsrc)
    _same_bits(cv, _np(tv)[_np(src)])                # return_index maps back to the input positions
    cv2, cf2 = clean_mesh(tv, tf, min_f=min_f, min_d=min_d)
    assert torch.equal(cv2.view(torch.int32), cv.view(torch.int32)) and torch.equal(cf2, cf)
    return _np(cv), _np(cf), _np(src)


def _check_decimate(v, f, target):
    from humangaussian_amd.meshclean import decimate_mesh
    dv, df, info = decimate_mesh(*_dev(v, f), target, return_info=True)
    wv, wf, winfo = ref.decimate(v, f, target)
    _same_bits(dv, wv)
    _same_bits(df, wf)
    if winfo is None:
        assert info is None
    else:
        assert info["grid"] == winfo["grid"] and info["cell"] == winfo["cell"] and info["input_faces"] == f.shape[0]
        assert info["probe_launches"] <= 10
    return _np(dv), _np(df), info


# ------------------------------------------------------------------------------------------------ components

COMPONENT_MESHES = {
    "two_tets": lambda: ref.two_tets(),
    "two_tets_interleaved": lambda: ref.two_tets(True),
    "strip_natural": lambda: ref.strip(2050, "natural"),
    "strip_reversed": lambda: ref.strip(2050, "reversed"),
    "strip_random": lambda: ref.strip(2050, "random", seed=3),
    "fan_1024": lambda: ref.fan_with_floaters(1023),
    "fan_1025": lambda: ref.fan_with_floaters(1024),
    "torus": lambda: ref.torus(),
}


@pytest.mark.parametrize("name", sorted(COMPONENT_MESHES))
def test_components_match_the_breadth_first_search(name):
    v, f = COMPONENT_MESHES[name]()
    rounds = _check_components(v, f)
    assert 1 <= rounds <= v.shape[0] + 5                  # the cap in the binding; in practice a dozen
    print(name, "rounds", rounds)


def test_a_face_with_a_repeated_index_connects_and_is_dropped():
    v, f = ref.two_tets()
    f = np.concatenate([f, [[0, 0, 4]], [[8, 8, 8]]])       # joins the tetrahedra; a face on the isolated vertex alone
    _check_components(v, f)
    from humangaussian_amd.meshclean import mesh_components
    labels, comp_faces, _ = mesh_components(*_dev(v, f))
    assert _np(labels).tolist() == [0] * 8 + [8] and _np(comp_faces)[[0, 8]].tolist() == [9, 1]
    cv, cf, src = _check_clean(v, f, 0, 0.0)
    assert cf.shape[0] == 8 and src.tolist() == list(range(8))


@pytest.mark.parametrize("index", [torch.int32, torch.int64])
def test_a_face_out_of_range_is_counted_and_raises(index):
    from humangaussian_amd.meshclean import clean_mesh, decimate_mesh, mesh_components
    v, f = ref.two_tets()
    f = np.concatenate([f, [[0, 4, 9]], [[-1, 1, 2]], [[0, 1, 2]]])
    tv, tf = _dev(v, f, index)
    for call in (lambda: mesh_components(tv, tf), lambda: clean_mesh(tv, tf), lambda: decimate_mesh(tv, tf, 3)):
        with pytest.raises(ValueError, match=r"2 faces index vertices outside \[0, 9\)"):
            call()
    if index == torch.int64:
        tf = tf.clone()
        tf[0, 0] = 2 ** 31
        with pytest.raises(ValueError, match="int32 range"):
            mesh_components(tv, tf)


def test_empty_meshes_launch_nothing():
    from humangaussian_amd.meshclean import clean_mesh, decimate_mesh, mesh_components
    v, f = ref.two_tets()
    tv, tf = _dev(v, f)
    none_v, none_f = tv[:0], tf[:0]
    labels, comp_faces, comp_diag2 = mesh_components(tv, none_f)                   # F == 0: every vertex on its own
    assert _np(labels).tolist() == list(range(9)) and not comp_faces.any() and not comp_diag2.any()
    for vv, ff in ((tv, none_f), (none_v, none_f)):
        cv, cf, src = clean_mesh(vv, ff, return_index=True)
        assert cv.shape == (0, 3) and cf.shape == (0, 3) and src.shape == (0,)
        assert cv.dtype == torch.float32 and cf.dtype == torch.int32 and src.dtype == torch.int32
        dv, df = decimate_mesh(vv, ff, 10)
        assert torch.equal(dv, vv) and df.shape == (0, 3)
    labels, comp_faces, comp_diag2 = mesh_components(none_v, none_f)
    assert labels.shape == (0,) and labels.dtype == torch.int32


# ------------------------------------------------------------------------------------------------ the keep rule

@pytest.mark.parametrize("n_rim", [1023, 1024])
def test_exactly_1024_and_1025_kept_vertices_and_faces(n_rim):
    """the compaction's scan-block boundary"""
    v, f = ref.fan_with_floaters(n_rim)
    cv, cf, src = _check_clean(v, f, 8, 0.0)
    assert cv.shape[0] == n_rim + 1 and cf.shape[0] == n_rim + 1


def test_min_f_is_inclusive():
    min_f = 64
    va, fa = ref.strip(min_f + 2)                                                # exactly min_f faces
    vb, fb = ref.strip(min_f + 1)                                                # min_f - 1
    v = np.concatenate([vb + np.float32([0, 4, 0]), va])
    f = np.concatenate([fb, fa + vb.shape[0]])
    cv, cf, src = _check_clean(v, f, min_f, 0.0)
    assert cf.shape[0] == min_f and src.tolist() == list(range(vb.shape[0], v.shape[0]))


def test_min_d_at_the_threshold_and_one_ulp_below():
    """Power-of-two coordinates: every fp32 operation of the rule is exact.  The mesh's box is 8 x 2^-10 x 0, so D2 = 64
    (64 + 2^-20 rounds to 64) and with min_d = 50 the threshold is 0.25 * 64 = 16.  Component 1 spans 4 along x:
    d2 = 16, kept.  Component 2 spans 4 - 2^-22 along x and 2^-10 along y: d2 = (16 - 2^-19) + 2^-20 = 16 - 2^-20, the
    float below 16: dropped."""
    below4 = np.nextafter(np.float32(4), np.float32(0))
    tiny = np.float32(2.0 ** -10)
    v = np.array([[0, 0, 0], [8, 0, 0], [1, 0, 0],                                # component 0: the mesh's extent
                  [2, 0, 0], [6, 0, 0], [3, 0, 0],                                # component 1: exactly the threshold
                  [0, 0, 0], [below4, tiny, 0], [2, 0, 0]], dtype=np.float32)       # component 2: one ulp below
    f = np.arange(9).reshape(3, 3)
    assert v[7, 0] - v[6, 0] == below4
    labels = ref.components_bfs(9, f)
    d2 = ref.component_stats(v, f, labels)[1]
    assert ref.keep_threshold(v, 50.0) == 16 and d2[3] == 16 and d2[6] == np.nextafter(np.float32(16), np.float32(0))
    cv, cf, src = _check_clean(v, f, 1, 50.0)
    assert src.tolist() == [0, 1, 2, 3, 4, 5]
    _check_clean(v, f, 1, 20.0)
    _check_clean(v, f, 1, 75.0)


def test_no_thresholds_drop_only_degenerate_faces_and_unreferenced_vertices():
    v, f = ref.fan_with_floaters(40)
    f = np.concatenate([f[:7], [[3, 3, 5]], f[7:], [[2, 9, 2]]])
    cv, cf, src = _check_clean(v, f, 0, 0.0)
    assert cf.shape[0] == f.shape[0] - 2
    assert src.tolist() == np.unique(f).tolist() and src.shape[0] == v.shape[0] - 5


# ------------------------------------------------------------------------------------------------ clustering

def test_vertices_exactly_on_cell_planes():
    v, f = ref.plane_grid(8)
    for target in (127, 64, 40, 9, 1):
        _check_decimate(v, f, target)


def test_a_mesh_without_extent_comes_back_without_faces():
    v = np.full((5, 3), 2.5, np.float32)
    f = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4], [0, 2, 4]])
    dv, df, info = _check_decimate(v, f, 2)
    assert dv.shape == (0, 3) and df.shape == (0, 3) and info["cell"] == 0.0


def test_all_vertices_in_one_cell_give_no_faces():
    v, f = ref.two_tets()
    dv, df, info = _check_decimate(v, f, 1)
    assert df.shape == (0, 3) and dv.shape == (0, 3)


def test_of_two_faces_on_one_vertex_set_the_lower_index_stays():
    v, f = ref.flipped_pair()
    dv, df, info = _check_decimate(v, f, 5)
    assert df.tolist() == [[0, 1, 2], [0, 1, 3]] and dv.shape == (4, 3)          # faces 0 and 2, orientation kept


def test_random_soup_just_below_its_face_count():
    """nearly every vertex has a cell of its own: the hash tables see real probing"""
    v, f = ref.random_soup(5000, 9000, seed=1)
    dv, df, info = _check_decimate(v, f, f.shape[0] - 1)
    assert info["grid"] > 64 and df.shape[0] > f.shape[0] // 2


@pytest.fixture(scope="module")
def sphere():
    """a marching-cubes sphere at resolution 32, from the project's own marching_cubes"""
    from humangaussian_amd.fields import marching_cubes
    ax = torch.linspace(-1, 1, 32, device=DEV)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v, f = marching_cubes(0.8 - torch.sqrt(x * x + y * y + z * z), 0.0)
    return _np(v), _np(f).astype(np.int64)


@pytest.fixture(scope="module")
def avatar_mesh():
    """the raw iso-surface of the procedural avatar at resolution 64"""
    from humangaussian_amd.fields import extract_mesh
    cloud = tuple(torch.as_tensor(a, device=DEV) for a in FC.avatar(6000, 4))
    v, f = extract_mesh(cloud, density_thresh=1, resolution=64)
    return _np(v), _np(f).astype(np.int64)


@pytest.mark.parametrize("which", ["F+1", "F", "F-1", "1000", "4", "0"])
def test_sphere_targets(sphere, which):
    from humangaussian_amd.meshclean import decimate_mesh
    v, f = sphere
    F = f.shape[0]
    assert F > 2000
    target = {"F+1": F + 1, "F": F, "F-1": F - 1, "1000": 1000, "4": 4, "0": 0}[which]
    dv, df, info = _check_decimate(v, f, target)
    if which in ("F+1", "F", "0"):                           # the input comes back bit for bit
        tv, tf = _dev(v, f)
        ov, of = decimate_mesh(tv, tf, target)
        assert torch.equal(ov.view(torch.int32), tv.view(torch.int32)) and torch.equal(of, tf) and info is None
    else:
        assert df.shape[0] <= target


def _properties(v, f, target):
    dv, df, info = _check_decimate(v, f, target)
    g, h = info["grid"], info["cell"]
    assert g == ref.choose_grid(v, f, target)[0]
    assert 0 < df.shape[0] <= target
    assert df.min() >= 0 and df.max() < dv.shape[0]
    assert (df[:, 0] != df[:, 1]).all() and (df[:, 1] != df[:, 2]).all() and (df[:, 0] != df[:, 2]).all()
    assert np.unique(np.sort(df, axis=1), axis=0).shape[0] == df.shape[0]          # no two faces on one vertex set
    assert np.array_equal(np.unique(df), np.arange(dv.shape[0]))                   # every vertex is referenced
    # every input vertex of a cell that has a new vertex lies within the cell's diagonal plus a lattice step of it
    _, _, rep = ref.cluster(v, f, g)                                               # (the smallest member of the vertex's cell)
    used = np.unique(rep[f][_surviving_mask(rep, f)])
    assert used.shape[0] == dv.shape[0]
    new_of_rep = np.full(v.shape[0], -1)
    new_of_rep[used] = np.arange(used.shape[0])
    has_new = new_of_rep[rep] >= 0
    emax = ref.box(v)[2]
    bound = h * np.sqrt(3.0) + float(emax) / ref.LATTICE
    dist = np.linalg.norm(v[has_new].astype(np.float64) - dv[new_of_rep[rep[has_new]]].astype(np.float64), axis=1)
    assert dist.max() <= bound, (dist.max(), bound)
    return dv, df, info


def _surviving_mask(rep, f):
    r = rep[f]
    return (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])


@pytest.mark.parametrize("target", [1000, 150])
def test_properties_on_the_sphere(sphere, target):
    _properties(*sphere, target)


@pytest.mark.parametrize("target", [4000, 500])
def test_properties_on_the_avatar(avatar_mesh, target):
    v, f = avatar_mesh
    assert f.shape[0] > 8000
    _properties(v, f, target)


# ------------------------------------------------------------------------------------------------ order and reproducibility

def test_face_order_changes_no_vertex_bit_and_calls_repeat(sphere):
    from humangaussian_amd.meshclean import clean_mesh, decimate_mesh
    v, f = sphere
    target = 700
    dv, df, info = _check_decimate(v, f, target)
    perm = np.random.default_rng(9).permutation(f.shape[0])
    pv, pf, pinfo = _check_decimate(v, f[perm], target)                            # (against the reference on the permuted list)
    assert np.array_equal(pv.view(np.int32), dv.view(np.int32)) and pinfo == info
    assert np.array_equal(np.unique(np.sort(pf, axis=1), axis=0), np.unique(np.sort(df, axis=1), axis=0))
    tv, tf = _dev(v, f)
    for _ in range(2):
        rv, rf = decimate_mesh(tv, tf, target)
        _same_bits(rv, dv)
        _same_bits(rf, df)
    cv, cf = clean_mesh(tv, tf, min_f=0, min_d=0.0)                                # a closed sphere: nothing to drop
    _same_bits(cv, v)
    _same_bits(cf, f.astype(np.int32))


# ------------------------------------------------------------------------------------------------ the public path

BLOB_AT, BLOB_RADIUS, BLOB_COUNT = (0.45, 0.3, 0.3), 0.03, 40


def _avatar_with_blob(n=6000, seed=4):
    """The procedural avatar plus 40 opaque Gaussians in a ball of radius 0.03 away from the body.  Chosen on the CPU with
    the numpy references (fields_reference.field + marching_cubes at resolution 64, mesh_clean_reference's components):
    the blob's iso-surface is a component of its own of 144 faces (>= min_f) whose squared box diagonal is 0.010 of the
    mesh's - a tenth of the diagonal, below min_d = 20 %, so it is the diagonal test that drops it; the body's two large
    components (trunk 0.78, head 0.045 of the squared diagonal; 0.04 is the bound) stay."""
    xyz, op, sc, rot = FC.avatar(n, seed)
    rng = np.random.default_rng(seed + 100)
    d = rng.normal(size=(BLOB_COUNT, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    blob = (np.asarray(BLOB_AT) + BLOB_RADIUS * d * rng.uniform(0, 1, (BLOB_COUNT, 1))).astype(np.float32)
    return (np.concatenate([xyz, blob]), np.concatenate([op, np.full((BLOB_COUNT, 1), 0.9, np.float32)]),
            np.concatenate([sc, np.full((BLOB_COUNT, 3), 0.02, np.float32)]),
            np.concatenate([rot, np.tile(np.float32([1, 0, 0, 0]), (BLOB_COUNT, 1))]))


class _Model:
    def __init__(self, cloud):
        self.get_xyz, self.get_opacity, self.get_scaling, self._rotation = (torch.as_tensor(a, device=DEV) for a in cloud)
        rng = np.random.default_rng(11)
        self._features_dc = torch.as_tensor(rng.normal(0, 1.0, (len(cloud[0]), 1, 3)).astype(np.float32), device=DEV)


def test_extract_clean_mesh_on_an_avatar_with_a_floater():
    from humangaussian_amd.animation import anchor_to_mesh
    from humangaussian_amd.fields import (extract_clean_mesh, extract_clean_mesh_attributes, extract_fields,
                                          extract_mesh, extract_mesh_attributes, gaussian_colors, marching_cubes)
    from humangaussian_amd.mesh import MeshIndex
    from humangaussian_amd.meshclean import mesh_components
    model = _Model(_avatar_with_blob())
    R, T = 64, 3000
    raw_v, raw_f = extract_mesh(model, resolution=R)
    # extract_mesh is today's path: marching_cubes + the transform
    occ = extract_fields(model, R)
    mv, mf = marching_cubes(occ, 1)
    mv = (mv / (R - 1.0) * 2 - 1) / model.scale + model.center
    assert torch.equal(raw_v.view(torch.int32), mv.view(torch.int32)) and torch.equal(raw_f, mf)

    def near_blob(v):
        return (v - torch.tensor(BLOB_AT, device=DEV)).norm(dim=1) < 3 * BLOB_RADIUS + 0.06

    labels, comp_faces, comp_diag2 = mesh_components(raw_v, raw_f)
    blob_labels = torch.unique(labels[near_blob(raw_v)])
    assert blob_labels.numel() == 1                                                # the blob is one component of its own
    blob = int(blob_labels[0])
    assert not near_blob(raw_v[labels != blob]).any() and near_blob(raw_v[labels == blob]).all()
    thr = ref.keep_threshold(_np(raw_v), 20.0)
    assert int(comp_faces[blob]) >= 64 and float(comp_diag2[blob]) < thr           # dropped by its diagonal
    body = int(torch.argmax(comp_faces))
    assert body != blob

    cv, cf = extract_clean_mesh(model, resolution=R)
    assert not near_blob(cv).any() and cf.shape[0] < raw_f.shape[0]
    clabels, ccomp_faces, _ = mesh_components(cv, cf)
    assert int(ccomp_faces.max()) == int(comp_faces[body])                         # the body's faces are all there
    wv, wf, _ = ref.clean(_np(raw_v), _np(raw_f), 64, 20.0)
    _same_bits(cv, wv)
    _same_bits(cf, wf)
    assert int((ccomp_faces > 0).sum()) == int(((comp_faces >= 64) & ~(comp_diag2 < thr) & (comp_faces > 0)).sum())

    dv, df = extract_clean_mesh(model, resolution=R, clean=True, decimate_target=T)
    assert 0 < df.shape[0] <= T and not near_blob(dv).any()
    wdv, wdf, _ = ref.decimate(wv, wf, T)
    _same_bits(dv, wdv)
    _same_bits(df, wdf)
    ov, of = extract_clean_mesh(model, resolution=R, clean=False, decimate_target=T)   # decimation alone keeps the floaters
    assert 0 < of.shape[0] <= T and near_blob(ov).any()

    nv, nf = extract_clean_mesh(model, resolution=R, clean=False)                  # both options off: the raw mesh
    assert torch.equal(nv.view(torch.int32), raw_v.view(torch.int32)) and torch.equal(nf, raw_f)

    index = MeshIndex(dv, df)                                                      # the result feeds the mesh stages
    anchors, keep, err = anchor_to_mesh(model.get_xyz, dv, df, max_error=0.05)
    assert keep.any() and torch.isfinite(err[keep]).all()
    del index

    av, af, normals, colors = extract_clean_mesh_attributes(model, resolution=R, clean=True, decimate_target=T)
    assert torch.equal(av.view(torch.int32), dv.view(torch.int32)) and torch.equal(af, df)
    n2 = (normals * normals).sum(dim=1)
    assert (((n2 - 1).abs() < 1e-5) | (n2 == 0)).all() and (n2 > 0).float().mean().item() > 0.9
    gc = gaussian_colors(model)
    assert colors.shape == av.shape and (colors >= gc.min() - 1e-5).all() and (colors <= gc.max() + 1e-5).all()
    # the raw call is untouched: today's result, bit for bit
    a0 = extract_mesh_attributes(model, resolution=R)
    assert torch.equal(a0[0].view(torch.int32), raw_v.view(torch.int32)) and torch.equal(a0[1], raw_f)
