"""CPU companion of tests/test_gpu_knn_boundaries.py: keeps its case table (tests/knn_reference.py::CASES) honest.  On the
float64 definition and the fp32 restatement of csrc/knn.hip alone - no device - every case is shown to reach the boundary it
is named for, under the host-exact grid rule (tests/gridfit_reference.py, pinned to csrc/gridscan.h by test_gridfit_cpu.py);
every cell index of every case, the non-finite ones included, is shown to lie inside the grid the scratch was sized for
BEFORE the case runs on a device; and the restated grid search equals the restated brute force bit for bit and the
definition within the sweep's tolerance.

The axis limit.  hgs_grid_fit accepts a grid only when ext / h < HGS_GRID_AXIS_MAX - 1 on every axis, so an accepted axis
has at most 4095 cells: the clamp to 4096 inside the loop can only survive if all 64 rounds of growth fail, which needs
ext / h0 > 4095 * 1.26^64 ~ 1e10, while the first cell edge of knn.hip gives ext / h0 <= cbrt(P / 2e-6) < 7e4 for any P the
binding takes.  g.max() == 4096 is therefore unreachable; what IS reachable, and what the two collinear cases pin, is the
limit itself: 4092 cells accepted as asked, and 4102 asked for, refused by the axis rule alone and regrown to 3256."""
import numpy as np
import pytest

import knn_reference as K

F = np.float32
RESTATE_MAX = 3000                     # points: the Python loops of grid_knn take seconds beyond


@pytest.fixture(scope="module")
def plans():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = K.grid_plan(K.points(name))
        return cache[name]
    return get


def asked_cells(pl):
    """cells per axis at the FIRST cell edge, before any growth"""
    return np.floor(pl.ext / pl.h0).astype(np.int64) + 1


def test_the_table_lists_every_boundary_of_the_issue():
    names = [c.name for c in K.CASES]
    assert len(set(names)) == len(names)
    assert [len(K.points(f"gauss_{P}")) for P in (1, 2, 3, 4, 8, 9, 255, 256, 257, 1023, 1024, 1025)] == \
        [1, 2, 3, 4, 8, 9, 255, 256, 257, 1023, 1024, 1025]
    for c in K.CASES:
        p = K.points(c.name)
        assert p.dtype == F and p.ndim == 2 and p.shape[1] == 3 and p.flags.c_contiguous, c.name
        bad = np.flatnonzero(~np.isfinite(p).all(1))
        assert tuple(bad) == tuple(c.bad), (c.name, bad)
    assert all(len(K.points(c.name)) == K.NONFINITE_P for c in K.CASES if c.bad)


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_every_cell_index_is_inside_the_grid(case, plans):
    """what hgs_k_knn_count / scan / scatter / search index with: 0 <= cell < ncells <= nc_max, for every input"""
    pl = plans(case.name)
    assert 1 <= pl.ncells <= pl.nc_max and (pl.g >= 1).all() and pl.g.max() <= 4095, (pl.g, pl.nc_max)
    assert (pl.cells >= 0).all() and (pl.cells < pl.g).all()
    assert pl.key.min() >= 0 and pl.key.max() < pl.ncells
    assert pl.count.sum() == len(K.points(case.name))
    assert np.isfinite(pl.h) and pl.h > 0 and np.isfinite(pl.inv_h)
    bad_axes = ~np.isfinite(K.points(case.name)).all(0)
    assert (pl.g[bad_axes] == 1).all() and (pl.ext[bad_axes] == 0).all()          # "that axis collapses"
    # the `reach` rule reads me - origin only on an axis with a cell beyond the block searched: never on a collapsed one,
    # the only ones whose origin or coordinates can be non-finite
    assert np.isfinite(pl.lo[~bad_axes]).all()


def test_fewer_than_three_neighbours_leave_empty_slots(plans):
    big = float(K.FLT_MAX)
    assert np.array_equal(K.expected("gauss_1"), [np.inf]) and np.array_equal(K.expected("gauss_2"), [np.inf, np.inf])
    w3 = K.expected("gauss_3")                  # (b0 + b1) + FLT_MAX does not overflow: b0 + b1 is far below ulp(FLT_MAX) / 2
    assert np.array_equal(w3, np.full(3, K.FLT_MAX / F(3.0)))
    assert np.isfinite(K.expected("gauss_4")).all() and K.expected("gauss_4").max() < 1e3 < big


def test_the_grid_switch_at_nine_points(plans):
    assert plans("gauss_8").ncells == 1 and plans("gauss_8").h0 is None
    assert plans("gauss_9").ncells > 1 and plans("gauss_9").h0 is not None


def test_the_fullest_cell_is_4096_and_4097(plans):
    a, b = plans("cell_4096"), plans("cell_4097")
    assert a.count.max() == K.CELL_MAX and b.count.max() == K.CELL_MAX + 1          # grid search | brute force
    assert np.array_equal(a.g, b.g) and a.ncells > 1 and a.rounds == b.rounds == 0
    for name, pl in (("cell_4096", a), ("cell_4097", b)):
        p = K.points(name)
        assert len(np.unique(p, axis=0)) == len(p)                                   # distinct points: no trivial distances
        assert np.sort(pl.count)[-2] <= 4                                            # the shell is sparse
    assert K.expected("cell_4096").min() > 0


def test_one_and_two_scan_blocks(plans):
    a, b = plans("cells_1024"), plans("cells_1025")
    assert a.ncells == K.SCAN_BLOCK and tuple(a.g) == (16, 8, 8)                     # the last element of the one block
    assert K.SCAN_BLOCK + 1 <= b.ncells <= 2 * K.SCAN_BLOCK and tuple(b.g) == (17, 8, 8)
    assert a.rounds == b.rounds == 0
    assert a.count[-1] > 0 and b.count[K.SCAN_BLOCK:].sum() > 0                      # points behind the block border


def test_all_equal_is_one_cell(plans):
    for name, n in (("all_equal_40", 40), ("all_equal_4097", 4097)):
        pl = plans(name)
        assert pl.ncells == 1 and pl.count.max() == n and pl.ext.max() == 0
        assert np.array_equal(K.expected(name), np.zeros(n, F))
    assert plans("all_equal_40").count.max() <= K.CELL_MAX < plans("all_equal_4097").count.max()


def test_the_cell_budget_makes_h_grow(plans):
    pl = plans("nc_max_outliers")
    asked = asked_cells(pl)
    assert int(np.prod(asked)) > pl.nc_max and asked.max() < 4095                   # the budget, not the axis limit
    assert pl.rounds >= 1 and pl.h > pl.h0 and pl.ncells <= pl.nc_max
    assert pl.count.max() <= K.CELL_MAX                                              # and still the grid search


def test_the_axis_limit_makes_h_grow(plans):
    a, b = plans("axis_below_limit"), plans("axis_limit")
    for pl in (a, b):
        assert int(np.prod(asked_cells(pl))) <= pl.nc_max                            # never the cell budget
        assert pl.count.max() <= K.CELL_MAX and tuple(pl.g[1:]) == (1, 1)
    assert a.rounds == 0 and 4090 <= a.g.max() <= 4095 and a.ext[0] / a.h0 < F(4095)
    assert b.ext[0] / b.h0 >= F(4095) and b.rounds == 1 and b.h == F(b.h0 * F(1.26))
    assert 4095 / 1.27 < b.g.max() <= 4095
    # the smallest such P in steps of 1000: one step down the axis rule is silent
    assert K.AXIS_P_ABOVE - K.AXIS_P_BELOW == 1000 and len(K.points("axis_limit")) == K.AXIS_P_ABOVE


def test_the_lattice_lies_on_the_cell_faces(plans):
    pl = plans("lattice")
    p = K.points("lattice")
    nodes = p[8:8 + K.LATTICE_N ** 3]
    assert tuple(pl.g) == (12, 12, 12) and pl.rounds == 0
    step = np.diff(np.unique(nodes[:, 0]))
    assert len(step) == K.LATTICE_N - 1 and np.abs(step - pl.h).max() <= 2 * np.spacing(F(1.0))    # spacing = 1 x cell edge
    k = np.round((nodes - pl.lo).astype(np.float64) / float(pl.h))
    assert np.abs((nodes - pl.lo).astype(np.float64) - k * float(pl.h)).max() <= 12 * np.spacing(F(1.0))      # on the faces
    assert np.array_equal(np.unique(k), np.arange(K.LATTICE_N))
    w = K.expected("lattice")[8 + (8 * 12 + 6) * 12 + 6]                             # an inner node that is there once: six ties at h^2
    assert abs(float(w) - float(pl.h) ** 2) <= 1e-6 * float(pl.h) ** 2
    far = K.points("lattice_1e3")
    assert far.min() > 998 and plans("lattice_1e3").ncells == pl.ncells


@pytest.mark.parametrize("case", [c for c in K.CASES if c.bad], ids=[c.name for c in K.CASES if c.bad])
def test_non_finite_points_drop_out_of_the_definition(case):
    p, want = K.points(case.name), K.expected(case.name)
    good = np.ones(len(p), bool)
    good[list(case.bad)] = False
    assert np.isposinf(want[~good]).all()                                            # every slot of theirs stays empty
    assert np.array_equal(want[good], K.mean_dist2_fp64(p[good]))                    # the finite points among themselves
    assert np.isfinite(want[good]).all() and not np.isnan(want).any()


RESTATED = [c for c in K.CASES if c.restate]


def test_what_is_not_restated_is_too_large_or_too_dense():
    for c in K.CASES:
        if not c.restate:
            assert len(K.points(c.name)) > RESTATE_MAX, c.name
        else:
            assert len(K.points(c.name)) <= RESTATE_MAX, c.name


@pytest.mark.parametrize("case", RESTATED, ids=[c.name for c in RESTATED])
def test_restated_grid_search_equals_restated_brute_force_and_the_definition(case):
    p = K.points(case.name)
    res = K.grid_knn(p)
    assert res is not None
    got, visited, g = res
    want = K.brute(p)
    assert got.tobytes() == want.tobytes(), (case.name, g)
    assert K.mismatch(got, K.expected(case.name)) is None, K.mismatch(got, K.expected(case.name))


def test_the_line_shortcut_equals_the_chunked_brute_force():
    rng = np.random.default_rng(2)
    x = rng.uniform(-3, 3, 700)
    x[10] = x[11]
    x[20] = x[21] = x[22] = x[23] = x[24]
    for n in (2, 3, 4, 5, 700):
        line = np.stack([np.full(n, 0.5), x[:n], np.full(n, -0.25)], 1).astype(F)
        tilt = line.copy()
        tilt[0, 0] = np.nextafter(F(0.5), F(1))                                      # two axes vary: the chunked form
        a, b = K.mean_dist2_fp64(line), K.mean_dist2_fp64(tilt)
        assert np.allclose(a, b, rtol=1e-6, atol=1e-13), n
        assert np.array_equal(np.isinf(a), np.isinf(b))


def test_the_definition_against_a_kd_tree():
    from scipy.spatial import cKDTree
    p = K.points("gauss_1025").astype(np.float64)
    d, _ = cKDTree(p).query(p, k=4)
    assert np.allclose(K.expected("gauss_1025"), (d[:, 1:] ** 2).mean(1), rtol=1e-6, atol=0)
