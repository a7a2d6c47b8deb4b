"""CPU tests of the photometric loss (include/hgs_rast.h: hgs_photometric_*; humangaussian_amd/photometric.py): the torch
restatement (tests/photometric_reference.py) against the recording of the reference's own l1_loss / ssim / psnr
(tests/golden/photometric_reference.npz), the header's backward formula against autograd of the restatement in float64,
and the C and Python surface without a GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import photometric_reference as PR
from humangaussian_amd import _lib, photometric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = np.load(os.path.join(ROOT, "tests", "golden", "photometric_reference.npz"))
CASES = sorted({k.split("/")[0] for k in FIXTURE.files if "/" in k})


def _restated(name, dtype):
    x, y = torch.from_numpy(FIXTURE[f"{name}/image"]), torch.from_numpy(FIXTURE[f"{name}/gt"])
    return PR.run(x, y, dtype, lam=float(FIXTURE["lambda_dssim"]))


def test_the_fixture_holds_what_the_issue_lists():
    assert CASES == ["chw", "near_equal", "random", "smooth", "tiny"] and float(FIXTURE["lambda_dssim"]) == 0.2
    assert FIXTURE["chw/image"].ndim == 3 and FIXTURE["chw/f64/psnr"].shape == (3, 1)          # psnr's 3-D rule: per channel
    assert FIXTURE["random/f64/psnr"].shape == (2, 1) and FIXTURE["random/f64/ssim_image"].shape == (2,)
    for name in CASES:
        assert FIXTURE[f"{name}/image"].size <= 2 * 3 * 37 * 53 and FIXTURE[f"{name}/image"].dtype == np.float32
        assert FIXTURE[f"{name}/f64/grad"].dtype == np.float64 and FIXTURE[f"{name}/f32/grad"].dtype == np.float32


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_in_float64(name):
    got = _restated(name, torch.float64)
    for k in ("loss", "l1", "ssim", "psnr", "ssim_image", "grad"):
        if f"{name}/f64/{k}" in FIXTURE.files:
            want = FIXTURE[f"{name}/f64/{k}"]
            assert got[k].shape == want.shape, k
            assert np.abs(got[k].numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), k


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_in_float32(name):
    got = _restated(name, torch.float32)
    for k in ("loss", "l1", "ssim"):                 # the same torch ops in the same order: 1 ulp at the most
        want = FIXTURE[f"{name}/f32/{k}"]
        assert got[k].dtype == torch.float32 and abs(float(got[k]) - float(want)) <= float(np.spacing(np.abs(want))), k
    # the gradient: autograd's graph is not node for node the reference's (mu * mu here, mu.pow(2) there), so its fp32
    # rounding may differ - by a small part of what the reference's own fp32 run is away from its fp64 run
    want, want64 = FIXTURE[f"{name}/f32/grad"], FIXTURE[f"{name}/f64/grad"]
    own = np.abs(want - want64).max()
    assert np.abs(got["grad"].numpy() - want).max() <= max(0.1 * own, 4 * np.finfo(np.float32).eps * np.abs(want).max())


def test_window_of_the_header_is_the_reference_s():
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    body = re.search(r"#define HGS_PM_WINDOW \{(.*?)\}", hdr, flags=re.S).group(1).replace("\\", " ")
    taps = [np.float32(t.strip().rstrip("f")) for t in body.split(",")]
    assert len(taps) == 11 == photometric.WINDOW_SIZE
    assert np.array_equal(np.array(taps, np.float32), PR.window1d().numpy())
    assert np.array_equal(np.array(_lib.PM_WINDOW, np.float32), PR.window1d().numpy())
    for name, value in (("HGS_PM_TILE_H", photometric.TILE_H), ("HGS_PM_TILE_W", photometric.TILE_W),
                        ("HGS_PM_FINISH_CHUNK", photometric.FINISH_CHUNK)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value
    assert photometric.TILE_H >= 11 and photometric.TILE_W >= 11 and photometric.MAX_DIM == _lib.SI_MAX_DIM


@pytest.mark.parametrize("kind", PR.CONTENT_KINDS)
def test_backward_formula_of_the_header_is_autograd_of_the_formulas(kind):
    """Filtering the three derivative maps with the SAME zero-padded window is the adjoint of the forward's filter: the
    window is symmetric.  Odd sizes narrower and wider than the window; float64, 1e-10 of max |gradient|."""
    for B, C, H, W in ((1, 2, 7, 9), (2, 3, 23, 17)):
        x, y = (t.double() for t in PR.content_case(kind, B, C, H, W, seed=3))
        x.requires_grad_(True)
        out = PR.formulas(x, y)
        for g_ssim, g_l1 in ((1.0, 0.0), (0.0, 1.0), (-0.2, 0.8)):
            want, = torch.autograd.grad(g_ssim * out["ssim"] + g_l1 * out["l1"], x, retain_graph=True)
            got = PR.filtered_gradient(x.detach(), y, g_ssim, g_l1)
            scale = max(float(want.abs().max()), 1.0 / x.numel())
            assert float((got - want).abs().max()) <= 1e-10 * scale, (kind, H, W, g_ssim, g_l1)


def test_c_surface_without_a_gpu():
    _lib.build()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 17 and lib.hgs_abi_version() == 17
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(hgs_photometric_\w+)\s*\(", hdr, flags=re.M))
    assert declared == {"hgs_photometric_forward", "hgs_photometric_backward", "hgs_photometric_workspace_bytes"}
    assert declared <= set(_lib.EXPORTS)
    # the struct of the header, member by member, against the ctypes mirror
    body = re.search(r"typedef struct hgs_photometric_args \{(.*?)\} hgs_photometric_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*([\w\s,]+);", body, flags=re.M) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [f[0] for f in _lib.HgsPhotometricArgs._fields_]
    # sizing is host arithmetic: per-tile partials and plane sums; the derivative maps only when a gradient is wanted
    B, C, H, W = 2, 3, 100, 70
    tiles = -(-H // photometric.TILE_H) * -(-W // photometric.TILE_W)
    small, full = lib.hgs_photometric_workspace_bytes(B, C, H, W, 0), lib.hgs_photometric_workspace_bytes(B, C, H, W, 1)
    assert small % 256 == 0 and full % 256 == 0
    assert 3 * B * C * (tiles * 4 + 8) <= small <= 3 * B * C * (tiles * 4 + 8) + 512
    assert 3 * B * C * H * W * 4 <= full - small < 3 * B * C * H * W * 4 + 256
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, _lib.SI_MAX_DIM + 1), (65536, 1, 1, 1), (8, 4, 8192, 8192)):
        assert lib.hgs_photometric_workspace_bytes(*bad, 1) == 0, bad
    assert lib.hgs_photometric_workspace_bytes(65535, 1, 1, 1, 1) > 0
    # refusals happen before any device work
    assert lib.hgs_photometric_forward(None, None) != 0 and lib.hgs_photometric_backward(None, None) != 0
    import ctypes
    args = _lib.HgsPhotometricArgs(B=1, C=3, H=8, W=8)
    assert lib.hgs_photometric_forward(ctypes.byref(args), None) != 0          # NULL pointers
    assert lib.hgs_photometric_backward(ctypes.byref(args), None) == 0         # no gradient given: nothing to do
    args.B = 0
    assert lib.hgs_photometric_backward(ctypes.byref(args), None) != 0


def test_python_contract_without_a_gpu():
    import humangaussian_amd
    assert humangaussian_amd.photometric_loss is photometric.photometric_loss
    assert humangaussian_amd.PhotometricLoss._fields == ("loss", "l1", "ssim", "psnr")
    # the reference's signatures
    assert list(inspect.signature(photometric.l1_loss).parameters) == ["network_output", "gt"]
    sig = inspect.signature(photometric.ssim)
    assert list(sig.parameters) == ["img1", "img2", "window_size", "size_average"]
    assert sig.parameters["window_size"].default == 11 and sig.parameters["size_average"].default is True
    assert list(inspect.signature(photometric.psnr).parameters) == ["img1", "img2"]
    assert inspect.signature(photometric.photometric_loss).parameters["lambda_dssim"].default == 0.2
    x, y = torch.rand(3, 12, 9), torch.rand(3, 12, 9)
    for call in (lambda: photometric.photometric_loss(x, y), lambda: photometric.l1_loss(x, y), lambda: photometric.ssim(x, y),
                 lambda: photometric.psnr(x, y), lambda: photometric.photometric_loss(x[None], y[None])):
        with pytest.raises(RuntimeError, match="HIP device"):                  # there is no CPU path
            call()
    for size in (7, 9, 13, 0):
        with pytest.raises(ValueError, match="window_size"):
            photometric.ssim(x, y, window_size=size)
    with pytest.raises(ValueError, match="requires grad"):
        photometric.photometric_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="requires grad"):
        photometric.ssim(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="shape"):
        photometric.photometric_loss(x, y[:, :, :8])
    with pytest.raises(ValueError, match=r"\(C, H, W\) or \(B, C, H, W\)"):
        photometric.photometric_loss(x[0], y[0])
    with pytest.raises(ValueError, match="size_average=False"):
        photometric.ssim(x, y, size_average=False)
    with pytest.raises(ValueError, match="device"):
        photometric.photometric_loss(x, y.to("meta"))
    with pytest.raises(ValueError, match="tensor"):
        photometric.photometric_loss(x, y.numpy())
    with pytest.raises(ValueError, match="planes"):
        photometric.photometric_loss(torch.empty(70000, 1, 1, 1, device="meta"), torch.empty(70000, 1, 1, 1, device="meta"))
    with pytest.raises(ValueError, match="pixels a side"):
        photometric.photometric_loss(torch.empty(1, 1, 1, 40000, device="meta"), torch.empty(1, 1, 1, 40000, device="meta"))
    with pytest.raises(ValueError, match="floating"):
        photometric.photometric_loss(torch.zeros(3, 4, 4, dtype=torch.int32), torch.zeros(3, 4, 4, dtype=torch.int32))
