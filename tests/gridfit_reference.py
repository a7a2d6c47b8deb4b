"""The grid rule of csrc/gridscan.h in numpy, fp32 where the device uses fp32: the ONE restatement the CPU tests of the k-NN
grid (test_knn_grid_cpu.py) and of the mesh index (test_mesh_query_cpu.py) build on; tests/test_gridfit_cpu.py compares it
exactly with a host build of the header's own functions."""
import numpy as np

F = np.float32
AXIS_MAX = 4096


def volume(ext):
    """hgs_grid_volume: flat axes count with 1e-3 of the longest."""
    floor_ext = F(F(ext.max()) * F(1e-3))
    return F(F(F(max(ext[0], floor_ext)) * F(max(ext[1], floor_ext))) * F(max(ext[2], floor_ext)))


def h0_knn(ext, P):
    """knn.hip: ~2 points per cell of the box volume"""
    return F(np.cbrt(F(F(F(2.0) * volume(ext)) / F(P))))


def h0_mesh(ext, nfaces):
    """mesh.hip: 8 F cells in the box volume"""
    return F(np.cbrt(F(volume(ext) / F(8.0 * nfaces))))


def fit(ext, h0, nc_max):
    """hgs_grid_fit -> (h, g, rounds of growth)"""
    ext, h = ext.astype(F), F(h0)
    for it in range(64):
        q = (ext / h).astype(F)
        g = np.clip(np.floor(q) + F(1.0), 1, AXIS_MAX).astype(np.int64)
        if int(np.prod(g)) <= nc_max and np.all(q < F(AXIS_MAX - 1)):
            break
        h = F(h * F(1.26))
    return h, g, it


def cell1(x, lo, inv_h, g):
    """hgs_grid_cell1 on arrays: x (..., 3) or one axis, lo and g alike"""
    c = np.floor(((x - lo).astype(F) * inv_h).astype(F))
    return np.fmin(np.fmax(c, F(0)), (g - 1).astype(F)).astype(np.int64)          # (fmaxf / fminf: NaN -> cell 0)


def grid(lo, ext, h0, nc_max):
    """What both setup kernels share behind their preconditions: (lo, h, 1 / h, g); ext.max() == 0 or h0 None: one cell."""
    if h0 is None or not ext.max() > 0:
        return lo, F(1.0), F(1.0), np.ones(3, np.int64)
    h, g, _ = fit(ext, h0, nc_max)
    return lo, h, F(F(1.0) / h), g
