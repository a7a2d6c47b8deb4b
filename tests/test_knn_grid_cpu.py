"""The CPU restatement (tests/knn_reference.py: numpy, fp32 where the device uses fp32) of the grid search of csrc/knn.hip - grid
from the bounding box, cell of a point, shells of cells, the `reach` stop rule - checked against the brute force on random, surface, planar,
collinear, duplicated and outlier-stretched clouds: the stop rule must never end a search before the true three nearest
neighbours have been seen.  (The HIP kernels themselves run in tests/test_gpu_api_contract.py against a k-d tree and against
the brute-force kernel, bit for bit.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_reference import brute, grid_knn  # noqa: E402  (the restatement itself: tests/knn_reference.py)


def clouds():
    rng = np.random.default_rng(0)
    yield "gauss", rng.normal(0, 0.4, (700, 3))
    th, u = rng.uniform(0, 2 * np.pi, 900), rng.uniform(-1, 1, 900)
    yield "sphere_surface", np.stack([np.sqrt(1 - u * u) * np.cos(th), np.sqrt(1 - u * u) * np.sin(th), u], 1) * 0.5
    yield "planar", np.concatenate([rng.uniform(-1, 1, (600, 2)), np.zeros((600, 1))], 1)
    yield "collinear", np.stack([rng.uniform(-3, 3, 300), np.zeros(300), np.zeros(300)], 1)
    dup = rng.normal(0, 0.2, (400, 3))
    dup[5] = dup[6]
    dup[50] = dup[51] = dup[52] = dup[53]
    yield "duplicates", dup
    out = rng.normal(0, 0.01, (500, 3))
    out[0] = (50.0, 0, 0)
    out[1] = (-50.0, 0.3, 0)
    yield "outliers", out                      # the box is stretched: almost everything falls into a few cells
    yield "tiny", rng.normal(0, 1, (5, 3))
    yield "all_equal", np.ones((40, 3)) * 0.25
    clus = np.concatenate([rng.normal((0, 0, 0), 0.01, (300, 3)), rng.normal((1, 1, 1), 0.3, (300, 3))])
    yield "two_scales", clus
    # clouds translated far from the world origin: ulp(|coord|) is no longer small against 1e-3 h
    far = rng.normal(0, 0.4, (600, 3)).astype(np.float32)
    yield "translated_1e3", far + np.float32(1.0e3)
    yield "translated_1e4", far + np.array([1.0e4, -1.0e4, 3.0e3], np.float32)


@pytest.mark.parametrize("name,pts", list(clouds()), ids=[n for n, _ in clouds()])
def test_grid_search_is_exact(name, pts):
    res = grid_knn(pts)
    assert res is not None
    got, visited, g = res
    want = brute(pts)
    assert np.array_equal(got, want), (name, np.abs(got - want).max(), g)


def test_grid_search_looks_at_a_small_neighbourhood_on_a_surface_cloud():
    rng = np.random.default_rng(1)
    th, u = rng.uniform(0, 2 * np.pi, 3000), rng.uniform(-1, 1, 3000)
    pts = np.stack([np.sqrt(1 - u * u) * np.cos(th), np.sqrt(1 - u * u) * np.sin(th), u], 1) * 0.5
    got, visited, g = grid_knn(pts)
    assert np.array_equal(got, brute(pts))
    assert visited < 0.05 * len(pts), visited          # candidates per point: a few dozen, not P
