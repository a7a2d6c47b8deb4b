"""CPU tests of the surface sampler's definition (tests/surface_sample_reference.py, the numpy restatement the HIP kernel
is held to bit for bit in tests/test_gpu_surface_sample.py): the generator's known answers, the honesty of the GPU cases,
the statistics of the samples, and the error paths of humangaussian_amd.surface that need no device."""
import math

import numpy as np
import pytest
import torch

import surface_sample_reference as ref

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    got = ref.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert tuple(int(x) for x in got) == want


def test_sample_words_are_philox_of_the_global_index():
    w = ref.words(3, seed=(5 << 32) | 9, offset=(1 << 32) - 1)
    for i in range(3):
        g = (1 << 32) - 1 + i
        want = ref.philox4x32_10(np.array([g & 0xffffffff, g >> 32, 0, 0], np.uint64), np.array([9, 5], np.uint64))
        assert np.array_equal(w[i], want)


def test_every_gpu_case_keeps_clear_of_the_table_boundaries():
    """No sample of any GPU case lies within F * 2^-50 * A of a boundary between two faces: four times the most that two
    summation orders, a last-bit difference in an area and the product u * A can move a boundary or t.  So the GPU test may
    demand the restatement's face of EVERY sample."""
    for name, F, variant, N in ref.cases():
        v, f = ref.soup(F, variant)
        r = ref.sample(v, f, N, seed=ref.SAMPLE_SEED)
        if N:
            assert r["margin"].min() > ref.honest_margin(F), (name, r["margin"].min(), ref.honest_margin(F))


def _chi2_sf(x, k):
    return float(torch.special.gammaincc(torch.tensor(k / 2.0, dtype=torch.float64), torch.tensor(x / 2.0, dtype=torch.float64)))


def test_faces_are_drawn_in_proportion_to_their_areas():
    v, f = ref.soup(64)
    n = 200000
    r = ref.sample(v, f, n, seed=ref.SAMPLE_SEED)
    expected = ref.face_areas(v, f) / r["area"] * n
    assert expected.min() > 100
    counts = np.bincount(r["face"], minlength=64)
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    p = _chi2_sf(chi2, 63)
    print(f"faces vs areas: chi2 {chi2:.1f}, p {p:.3f}, smallest expected count {expected.min():.0f}")
    assert p > 1e-6


def test_samples_fill_the_four_sub_triangles_equally():
    v, f = ref.soup(64)
    n = 200000
    u, vv, w = ref.sample(v, f, n, seed=ref.SAMPLE_SEED)["uvw"].astype(np.float64).T
    part = np.where(u > 0.5, 0, np.where(vv > 0.5, 1, np.where(w > 0.5, 2, 3)))
    counts = np.bincount(part, minlength=4)
    chi2 = float(((counts - n / 4) ** 2 / (n / 4)).sum())
    p = _chi2_sf(chi2, 3)
    print(f"sub-triangles: counts {counts.tolist()}, p {p:.3f}")
    assert p > 1e-6


def test_barycentric_coordinates_are_exact():
    v, f = ref.soup(64)
    uvw = ref.sample(v, f, 100000, seed=3)["uvw"]
    assert uvw.dtype == np.float32 and uvw.min() >= 0.0 and uvw.max() <= 1.0
    assert np.array_equal((uvw[:, 0] + uvw[:, 1]) + uvw[:, 2], np.ones(len(uvw), np.float32))      # in fp32, no rounding
    assert np.array_equal(uvw.astype(np.float64).sum(1), np.ones(len(uvw)))


@pytest.mark.parametrize("variant", ["zero_area", "nan_vertex", "bad_index"])
def test_a_face_without_area_is_never_drawn(variant):
    F = 65
    v, f = ref.soup(F, variant)
    r = ref.sample(v, f, 100000, seed=ref.SAMPLE_SEED)
    dead = (0, F // 2, F - 1) if variant == "zero_area" else (F // 2,)
    assert r["num_positive"] == F - len(dead)
    assert not np.isin(r["face"], dead).any()
    assert np.isfinite(r["points"]).all()


def test_offset_calls_are_slices_of_the_larger_call():
    v, f = ref.soup(65)
    whole = ref.sample(v, f, 1000, seed=11, offset=5)
    part = ref.sample(v, f, 300, seed=11, offset=5 + 417)
    for k in ("face", "uvw", "points"):
        assert np.array_equal(whole[k][417:717], part[k])


def test_another_seed_gives_other_faces():
    v, f = ref.soup(1024)
    a, b = ref.sample(v, f, 1000, seed=1)["face"], ref.sample(v, f, 1000, seed=2)["face"]
    assert (a != b).mean() > 0.9


def test_error_paths_raise_before_any_device_call():
    from humangaussian_amd import surface
    v, f = ref.soup(4)
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        surface.SurfaceSampler(v, f.reshape(-1))
    with pytest.raises(ValueError, match=r"\(V, 3\)"):
        surface.SurfaceSampler(v[:, :2], f)
    with pytest.raises(ValueError, match="no faces"):
        surface.SurfaceSampler(v, np.zeros((0, 3), np.int32))
    with pytest.raises(RuntimeError, match="HIP device"):
        surface.SurfaceSampler(torch.from_numpy(v), torch.from_numpy(f))
    for bad in (-1, 1 << 64, 1.5, None):
        with pytest.raises(ValueError, match="seed"):
            surface.sample_surface(v, f, 10, seed=bad)
    with pytest.raises(ValueError, match="n must be"):
        surface.sample_surface(v, f, -1)
    with pytest.raises(ValueError, match="max_sh_degree"):
        surface.create_from_points(torch.zeros(4, 3), max_sh_degree=-1)
    with pytest.raises(ValueError, match=r"\(P, 3\)"):
        surface.create_from_points(torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        surface.create_from_points(torch.zeros(4, 3))


def test_the_package_exports_the_new_names():
    import humangaussian_amd as h
    for name in ("SurfaceSampler", "sample_surface", "create_from_points", "create_from_pcd", "init_from_body"):
        assert name in h.__all__ and callable(getattr(h, name))
    assert math.isclose(float(np.float32(np.log(np.float64(np.float32(0.1) / np.float32(0.9))))), -2.1972246, rel_tol=1e-6)
