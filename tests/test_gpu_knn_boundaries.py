"""The 3-nearest-neighbour kernels of csrc/knn.hip (`distCUDA2`: box, grid fit, counting sort, device-wide scan, ring search,
brute-force fallback) at their boundaries, against the float64 definition of tests/knn_reference.py.  One table
(knn_reference.CASES); tests/test_knn_boundaries_cpu.py proves without a device that each case reaches the boundary it is named
for and that every cell index it produces - the non-finite inputs included - lies inside the grid.  Every case must hold:

* the grid form and the brute force return the same bits;
* both are within rtol 2e-5 / atol 1e-9 of the definition where it is finite, and +inf exactly where it is +inf (fewer than
  two neighbours at a finite distance: the empty slots hold FLT_MAX and the fp32 sum overflows);
* no NaN in the output, whatever the input: a candidate at a NaN or infinite distance is ignored, so a point with a
  non-finite coordinate gets +inf and leaves every other point's value what it is without it.

Before non-finite points were taken out of the search (csrc/knn.hip::knn_finite: as candidates they sit at +inf, as queries
they get +inf) a NaN distance went through the branch-free insert as a second copy of the nearest distance, (2 d0 + d1) / 3
in place of (d0 + d1 + d2) / 3.  On this table: one NaN coordinate among 600 points put 217 values of the brute force off by
up to 75 % and 19 - 69 values of the grid search (the points whose rings met the bad one) by up to 57 %; a point that is NaN
on every axis (one cell) 449 and 597 of 599 in two runs (the order inside a cell is arbitrary); the two forms disagreed with
each other in all three.  Infinities alone did no harm.

Then the input forms of the binding (torch_binding.cpp::knn_mean_dist2 through f32c): strided, offset, fp64, fp16 and
requires_grad inputs equal the contiguous fp32 call bit for bit; a wrong shape or a CPU tensor raises."""
import numpy as np
import pytest
import torch

import knn_reference as K
from humangaussian_amd.knn import distCUDA2

pytestmark = pytest.mark.gpu


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_boundary_case_matches_the_fp64_definition(case):
    pts, want = K.points(case.name), K.expected(case.name)
    p = torch.from_numpy(pts.copy()).cuda()
    grid, brute = distCUDA2(p), distCUDA2(p, brute_force=True)
    assert grid.shape == brute.shape == (len(pts),) and grid.dtype == torch.float32
    g, b = grid.cpu().numpy(), brute.cpu().numpy()
    err_g, err_b = K.mismatch(g, want), K.mismatch(b, want)
    print(f"{case.name}: grid {err_g or 'ok'} | brute {err_b or 'ok'} | same bits {torch.equal(bits(grid), bits(brute))}")
    assert torch.equal(bits(grid), bits(brute)), (case.name, case.boundary)
    assert err_g is None, (case.name, case.boundary, err_g)
    assert err_b is None, (case.name, case.boundary, err_b)
    if case.bad:
        bad = list(case.bad)
        good = np.setdiff1d(np.arange(len(pts)), bad)
        assert np.isposinf(g[bad]).all()
        # the finite points: the cloud without the bad ones (same tolerance, against the definition on that cloud)
        assert K.mismatch(g[good], K.mean_dist2_fp64(pts[good])) is None


@pytest.fixture(scope="module")
def cloud():
    pts = K.points("gauss_1025")
    p = torch.from_numpy(pts.copy()).cuda()
    return p, distCUDA2(p), distCUDA2(p, brute_force=True)


@pytest.mark.parametrize("brute_force", [False, True], ids=["grid", "brute"])
def test_input_forms_equal_the_contiguous_fp32_call(cloud, brute_force):
    p, grid, brute = cloud
    want = brute if brute_force else grid
    P = len(p)
    wide = torch.full((P, 4), float("nan"), device="cuda")
    wide[:, :3] = p
    forms = {"slice of (P, 4)": wide[:, :3]}
    wide_t = torch.full((3, P), float("nan"), device="cuda")
    wide_t.copy_(p.t())
    forms["transposed storage"] = wide_t.t()
    longer = torch.full((P + 7, 3), float("nan"), device="cuda")
    longer[5:5 + P] = p
    forms["storage offset"] = longer[5:5 + P]
    forms["every second row"] = torch.stack([p, torch.full_like(p, float("nan"))], 1).reshape(2 * P, 3)[::2]
    forms["fp64"] = p.double()
    forms["requires_grad"] = p.clone().requires_grad_(True)
    assert not forms["slice of (P, 4)"].is_contiguous() and not forms["transposed storage"].is_contiguous()
    assert forms["storage offset"].storage_offset() == 15 and not forms["every second row"].is_contiguous()
    for name, x in forms.items():
        got = distCUDA2(x, brute_force=brute_force)
        assert got.dtype == torch.float32 and not got.requires_grad and got.is_contiguous(), name
        assert torch.equal(bits(got), bits(want)), name
    # fp16: the values after the conversion to fp32, nothing else
    h = p.half()
    assert torch.equal(bits(distCUDA2(h, brute_force=brute_force)), bits(distCUDA2(h.float(), brute_force=brute_force)))
    # the input itself is left alone
    assert torch.equal(wide[:, :3], p) and bool(torch.isnan(wide[:, 3]).all())


@pytest.mark.parametrize("brute_force", [False, True], ids=["grid", "brute"])
def test_wrong_shapes_and_cpu_tensors_raise(brute_force):
    for shape in ((12,), (12, 3, 1), (12, 2), (12, 4), (3, 12), ()):
        with pytest.raises(RuntimeError, match=r"points must have dimensions \(num_points, 3\)"):
            distCUDA2(torch.zeros(shape, device="cuda"), brute_force=brute_force)
    with pytest.raises(RuntimeError, match="must live on a HIP device"):
        distCUDA2(torch.zeros(12, 3), brute_force=brute_force)
    assert distCUDA2(torch.zeros(0, 3, device="cuda"), brute_force=brute_force).shape == (0,)
