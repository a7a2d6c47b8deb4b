"""csrc/gridscan.h's grid rule - hgs_grid_volume, hgs_grid_fit, hgs_grid_cell1 - built for the host with g++
(tests/gridfit_host.cpp: the SAME functions the kernels of knn.hip and mesh.hip compile) against the numpy restatement
tests/gridfit_reference.py that the CPU tests of both users search with: exact equality, for both first-edge rules."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridfit_reference as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gridfit") / "gridfit_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", os.path.join(ROOT, "tests", "gridfit_host.cpp"),
                           "-o", so])
    L = ctypes.CDLL(so)
    L.hgs_grid_volume_host.restype = ctypes.c_float
    L.hgs_grid_volume_host.argtypes = [ctypes.c_void_p, ctypes.c_float]
    L.hgs_grid_fit_host.restype = ctypes.c_float
    L.hgs_grid_fit_host.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_uint32, ctypes.c_void_p]
    L.hgs_grid_cell1_host.restype = None
    L.hgs_grid_cell1_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    return L


def clouds():
    rng = np.random.default_rng(3)
    yield "random", rng.normal(0, 0.4, (700, 3)), None
    yield "random_far", rng.normal(0, 0.4, (500, 3)) + np.array([1.0e3, -2.0e3, 5.0e2]), None
    yield "planar", np.concatenate([rng.uniform(-1, 1, (600, 2)), np.full((600, 1), 0.25)], 1), None
    yield "collinear", np.stack([rng.uniform(-3, 3, 300), np.zeros(300), np.zeros(300)], 1), None
    yield "small_budget", rng.uniform(-1, 1, (5000, 3)), 64          # nc_max far below the cells h0 asks for: h grows
    # one long axis and enough points / faces that BOTH first edges ask for more than 4095 cells on it (ext / h0 =
    # cbrt(n / 2e-6) = 4217 for knn, cbrt(8e6 n) = 10627 for mesh): the per-axis limit makes h grow, not the cell budget
    yield "long_axis", rng.uniform(-1, 1, (150_000, 3)) * np.array([500.0, 0.01, 0.01]), None


def h0_rules(ext, n):
    # (rule, h0, nc_max): knn.hip with P = n points, mesh.hip with F = n faces
    yield "knn", G.h0_knn(ext, n), min(max(64, 2 * n), 1 << 22)
    yield "mesh", G.h0_mesh(ext, n), min(max(16 * n, 64), 1 << 22)


@pytest.mark.parametrize("name,pts,budget", list(clouds()), ids=[c[0] for c in clouds()])
def test_host_build_of_the_grid_rule_equals_the_numpy_restatement(lib, name, pts, budget):
    pts = pts.astype(F)
    lo = pts.min(0)
    ext = np.ascontiguousarray((pts.max(0) - lo).astype(F))
    vol = lib.hgs_grid_volume_host(ext.ctypes.data, ctypes.c_float(ext.max()))
    assert F(vol) == G.volume(ext) and vol > 0
    for rule, h0, nc_max in h0_rules(ext, len(pts)):
        nc_max = budget or nc_max
        g = np.zeros(3, np.uint32)
        h = F(lib.hgs_grid_fit_host(ext.ctypes.data, ctypes.c_float(h0), nc_max, g.ctypes.data))
        want_h, want_g, rounds = G.fit(ext, h0, nc_max)
        assert h.tobytes() == want_h.tobytes() and list(g) == list(want_g), (rule, h, want_h, g, want_g)
        assert int(np.prod(want_g)) <= nc_max and want_g.max() <= 4096 and rounds < 63, (rule, want_g, rounds)
        if name == "small_budget":
            assert rounds >= 3, (rule, rounds)
        if name == "long_axis":
            assert ext[0] / h0 > 4095 and rounds >= 1 and want_g.max() <= 4096 and int(np.prod(want_g)) < nc_max // 8, (rule, rounds, want_g)
        if name in ("planar", "collinear"):
            assert (want_g == 1).sum() == (ext == 0).sum(), (rule, want_g)      # flat axes: one cell
        inv_h = F(F(1.0) / h)
        # every point, points outside the box, non-finite ones
        probe = np.concatenate([pts, pts[:50] * F(3.0) + F(7.0), np.array([[np.nan, np.inf, -np.inf]] * 2, F)]).astype(F)
        for a in range(3):
            x = np.ascontiguousarray(probe[:, a])
            out = np.zeros(len(x), np.int32)
            lib.hgs_grid_cell1_host(len(x), x.ctypes.data, ctypes.c_float(lo[a]), ctypes.c_float(inv_h), int(g[a]), out.ctypes.data)
            with np.errstate(invalid="ignore"):
                want = G.cell1(x, lo[a], inv_h, want_g[a:a + 1])
            assert np.array_equal(out, want), (rule, a)
            assert out.min() >= 0 and out.max() <= g[a] - 1
