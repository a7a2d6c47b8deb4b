"""Mesh cleaning and decimation without a GPU: the numpy restatement against itself (breadth-first search against the
emulated label rounds, the bisection against its budget), the C entry points' argument checks and sizing functions, and
the public signatures."""
import ctypes
import inspect

import numpy as np
import pytest

import mesh_clean_reference as ref
from humangaussian_amd import _lib

MESHES = {
    "two_tets": lambda: ref.two_tets(),
    "two_tets_interleaved": lambda: ref.two_tets(True),
    "strip_natural": lambda: ref.strip(2050, "natural"),
    "strip_reversed": lambda: ref.strip(2050, "reversed"),
    "strip_random": lambda: ref.strip(2050, "random", seed=3),
    "torus": lambda: ref.torus(),
    "fan_1024": lambda: ref.fan_with_floaters(1023),
    "fan_1025": lambda: ref.fan_with_floaters(1024),
    "soup": lambda: ref.random_soup(500, 900),
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_bfs_and_rounds_agree(name):
    v, f = MESHES[name]()
    V = v.shape[0]
    labels = ref.components_bfs(V, f)
    rounds_labels, rounds = ref.components_rounds(V, f)
    assert np.array_equal(labels, rounds_labels)
    assert rounds <= V + 1                       # the binding's cap is V + 1 rounds (plus the rounds of one host read)
    assert rounds <= 16, rounds                   # with the roots hooked: a dozen rounds even on the 2 050-vertex chains
    assert (labels <= np.arange(V)).all() and np.array_equal(labels[labels], labels)


def test_rounds_without_root_hooking_are_many():
    v, f = ref.strip(2050, "random", seed=3)
    labels, rounds = ref.components_rounds(v.shape[0], f, hook_roots=False)
    assert np.array_equal(labels, ref.components_bfs(v.shape[0], f))
    assert rounds > 3 * ref.components_rounds(v.shape[0], f)[1]


def test_component_stats_of_two_tets():
    v, f = ref.two_tets()
    labels = ref.components_bfs(9, f)
    assert labels.tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8]
    comp_faces, comp_diag2 = ref.component_stats(v, f, labels)
    assert comp_faces.tolist() == [4, 0, 0, 0, 4, 0, 0, 0, 0]
    assert comp_diag2[0] == 3.0 and comp_diag2[4] == 0.75 and comp_diag2[8] == 0.0


def test_out_of_range_faces_are_ignored():
    v, f = ref.two_tets()
    bad = np.concatenate([f, [[0, 4, 9]], [[-1, 1, 2]]])
    assert np.array_equal(ref.components_bfs(9, bad), ref.components_bfs(9, f))
    assert ref.valid_faces(9, bad).sum() == 8


@pytest.mark.parametrize("name", ["torus", "soup", "fan_1025", "strip_random"])
def test_bisection_never_exceeds_its_target(name):
    v, f = MESHES[name]()
    F = f.shape[0]
    for target in (F - 1, F // 2, F // 7, 10, 1):
        g, probes = ref.choose_grid(v, f, target)
        assert 1 <= g <= ref.G_MAX and probes == 10
        assert ref.surviving(v, f, g) <= target
        nv, nf, info = ref.decimate(v, f, target)
        assert nf.shape[0] <= target and info["grid"] == g
        if nf.size:
            assert nf.min() >= 0 and nf.max() < nv.shape[0]
            assert np.array_equal(np.unique(nf), np.arange(nv.shape[0]))


def test_decimate_no_op_cases():
    v, f = ref.torus()
    for target in (0, -3, f.shape[0], f.shape[0] + 1):
        nv, nf, info = ref.decimate(v, f, target)
        assert info is None and np.array_equal(nv, v) and np.array_equal(nf, f)


def test_clean_drops_small_components():
    v, f = ref.fan_with_floaters(1023)
    cv, cf, src = ref.clean(v, f, min_f=8, min_d=0.0)
    assert cv.shape[0] == 1024 and cf.shape[0] == 1024
    assert np.array_equal(cv, v[src]) and (np.diff(src) > 0).all()
    assert np.array_equal(np.unique(cf), np.arange(1024))


def _args(**kw):
    a = _lib.HgsMeshcleanArgs()
    for k, val in kw.items():
        setattr(a, k, val)
    return a


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    info = _lib.HgsMeshcleanInfo()
    g = (ctypes.c_int32 * 3)(2, 0, 0)
    calls = [
        lambda a: lib.hgs_meshclean_begin(a, None),
        lambda a: lib.hgs_meshclean_rounds(a, 4, None, None),
        lambda a: lib.hgs_meshclean_components(a, None),
        lambda a: lib.hgs_meshclean_clean_mark(a, None),
        lambda a: lib.hgs_meshclean_clean_emit(a, ctypes.byref(info), None),
        lambda a: lib.hgs_meshclean_count(a, g, None, None),
        lambda a: lib.hgs_meshclean_decimate_mark(a, 2, None),
        lambda a: lib.hgs_meshclean_decimate_emit(a, ctypes.byref(info), None),
    ]
    for call in calls:
        assert call(None) == -1                                     # args == NULL
        assert call(ctypes.byref(_args(V=-1, F=4))) == -1           # negative sizes
        assert call(ctypes.byref(_args(V=4, F=-1))) == -1
        assert call(ctypes.byref(_args(V=4, F=4))) == -1            # NULL arrays (and info)
        assert call(ctypes.byref(_args(V=(1 << 29) + 1, F=4))) == -1
    ok = _args(V=4, F=4, vertices=8, faces=8, info=8, scratch=8, labels=8, comp_faces=8, comp_diag2=8)   # never dereferenced:
    assert lib.hgs_meshclean_rounds(ctypes.byref(ok), 0, 8, None) == -1                                # refused before
    assert lib.hgs_meshclean_rounds(ctypes.byref(ok), 65, 8, None) == -1
    assert lib.hgs_meshclean_decimate_mark(ctypes.byref(ok), 0, None) == -1
    assert lib.hgs_meshclean_decimate_mark(ctypes.byref(ok), _lib.MESHCLEAN_G_MAX + 1, None) == -1
    big = (ctypes.c_int32 * 3)(_lib.MESHCLEAN_G_MAX + 1, 0, 0)
    assert lib.hgs_meshclean_count(ctypes.byref(ok), big, 8, None) == -1
    assert lib.hgs_meshclean_clean_emit(ctypes.byref(ok), None, None) == -1
    for field, val in (("error", 1), ("bad_faces", 1), ("num_vertices", 5), ("num_faces", 5)):
        bad_info = _lib.HgsMeshcleanInfo()
        setattr(bad_info, field, val)
        assert lib.hgs_meshclean_clean_emit(ctypes.byref(ok), ctypes.byref(bad_info), None) == -1
        assert lib.hgs_meshclean_decimate_emit(ctypes.byref(ok), ctypes.byref(bad_info), None) == -1


def test_scratch_size_is_monotone_and_zero_for_impossible_sizes():
    lib = _lib.load()
    size = lib.hgs_meshclean_scratch_bytes
    assert size(-1, 4) == 0 and size(4, -1) == 0 and size((1 << 29) + 1, 0) == 0 and size(0, (1 << 29) + 1) == 0
    assert size(0, 0) > 0 and size(1 << 29, 1 << 29) > 0
    steps = [0, 1, 31, 32, 33, 1023, 1024, 1025, 5000, 1 << 20, (1 << 20) + 1, 1 << 29]
    for fixed in (0, 1000):
        by_v = [size(n, fixed) for n in steps]
        by_f = [size(fixed, n) for n in steps]
        assert by_v == sorted(by_v) and by_f == sorted(by_f)
    # the tables alone: a power of two of at least twice the items, 4 bytes a slot
    assert size(5000, 9000) >= 4 * (16384 + 32768)


def test_struct_sizes_and_abi_version():
    assert _lib.ABI_VERSION == 17
    assert _lib.load().hgs_abi_version() == 17
    assert ctypes.sizeof(_lib.HgsMeshcleanInfo) == 64
    assert ctypes.sizeof(_lib.HgsMeshcleanArgs) == 96


def test_public_signatures():
    """extract_mesh and extract_mesh_attributes keep their signatures (other tests pin them exactly); the finished
    mesh comes from two new functions that take the old parameters in their old positions"""
    from humangaussian_amd import fields, meshclean
    import humangaussian_amd

    p = list(inspect.signature(fields.extract_mesh).parameters.values())                   # untouched
    assert [(q.name, q.default) for q in p[1:]] == [("density_thresh", 1), ("resolution", 128)]
    p = list(inspect.signature(fields.extract_clean_mesh).parameters.values())
    assert [q.name for q in p[:3]] == ["model", "density_thresh", "resolution"]
    assert [q.default for q in p[1:3]] == [1, 128]
    assert {q.name: q.default for q in p[3:]} == {"clean": True, "decimate_target": 0, "min_f": 64, "min_d": 20.0}
    p = list(inspect.signature(fields.extract_mesh_attributes).parameters.values())        # untouched
    assert [(q.name, q.default) for q in p[1:]] == [("density_thresh", 1), ("resolution", 128), ("colors", None)]
    p = list(inspect.signature(fields.extract_clean_mesh_attributes).parameters.values())
    assert [q.name for q in p[:4]] == ["model", "density_thresh", "resolution", "colors"]
    assert [q.default for q in p[1:4]] == [1, 128, None]
    assert {q.name: q.default for q in p[4:]} == {"clean": True, "decimate_target": 0, "min_f": 64, "min_d": 20.0}
    p = inspect.signature(meshclean.clean_mesh).parameters
    assert p["min_f"].default == 64 and p["min_d"].default == 20.0 and p["return_index"].default is False
    for name in ("mesh_components", "clean_mesh", "decimate_mesh"):
        assert getattr(humangaussian_amd, name) is getattr(meshclean, name)


def test_cpu_tensors_raise_the_device_error():
    import torch
    from humangaussian_amd.meshclean import clean_mesh, decimate_mesh, mesh_components

    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for call in (lambda: mesh_components(v, f), lambda: clean_mesh(v, f), lambda: decimate_mesh(v, f, 1)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
