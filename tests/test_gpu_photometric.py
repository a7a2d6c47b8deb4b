"""The photometric loss on the GPU (humangaussian_amd.photometric; csrc/photometric.hip) against the float64 run of its
formulas (tests/photometric_reference.py).  The gate of every quantity of every case is the distance of the float32 run
of those formulas on the CPU from the float64 run ON THE SAME INPUT, times 4 for the different order the 121 taps are
added in, with floors: 1e-6 on the scalars (relative to max(1, |value|): psnr is tens of dB, where fp32 itself resolves
2e-6) and 1e-5 on the gradient measure max |g - g64| / max(max |g64|, 1 / numel).  Nothing of a gate comes from the
kernel.  Shapes are the smallest that reach a halo, a partial tile, a window wider than the image, a second plane or
tile, and the boundaries of the finalize step.  HGS_WRITE_PROFILES=1 records kernel distance over reference distance per
case in profiles/photometric_parity.json."""
import ctypes
import functools
import json
import os

import pytest
import torch

import photometric_reference as PR
from humangaussian_amd import _lib, photometric
from humangaussian_amd import photometric_loss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
TH, TW, CHUNK = photometric.TILE_H, photometric.TILE_W, photometric.FINISH_CHUNK

SIZES = [(1, 1), (1, 40), (40, 1), (5, 7), (10, 11), (11, 10), (12, 16), (16, 17), (17, 33), (31, 32), (33, 31), (37, 53)]
SIZES += [(TH + d, 40) for d in (-1, 0, 1)] + [(40, TW + d) for d in (-1, 0, 1)]
SIZES += [(2 * TH + d, 40) for d in (-1, 1)] + [(40, 2 * TW + d) for d in (-1, 1)]
SIZES += [(TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH - 1, 2 * TW + 1), (2 * TH + 1, 2 * TW - 1), (2 * TH, 2 * TW)]
PLANES = [(1, 3), (2, 3), (3, 1), (1, 4)]
assert TH == 32 and TW == 32 and CHUNK == 64, "the boundary table below is written for these"
# tiles per plane one below, at and one above the stride of the finalize step; more planes than its 16 waves; many workgroups
BOUNDARIES = {"tiles_63": (1, 1, 7 * TH, 9 * TW), "tiles_64": (1, 1, 8 * TH, 8 * TW), "tiles_65": (1, 1, 5 * TH, 13 * TW - 3),
              "tiles_129": (1, 2, 3 * TH - 5, 43 * TW), "planes_16": (4, 4, 9, 8), "planes_17": (17, 1, 8, 9),
              "many_workgroups": (1, 3, 256, 320)}


@functools.lru_cache(maxsize=None)
def _reference(kind, B, C, H, W, seed):
    """inputs and the two CPU runs of a case: computed once, shared, never modified"""
    x, y = PR.content_case(kind, B, C, H, W, seed)
    r64, r32 = PR.run(x, y, torch.float64), PR.run(x, y, torch.float32)
    r64["psnr_chw"], r32["psnr_chw"] = PR.psnr(x[0].double(), y[0].double()), PR.psnr(x[0], y[0])
    gates = PR.gates(r32, r64)
    gates["psnr_chw"] = max(PR.MARGIN * PR.scalar_distance(r32["psnr_chw"], r64["psnr_chw"]), PR.SCALAR_FLOOR)
    return x, y, r64, r32, gates


def _run_hip(x, y, lam=0.2):
    img, gt = x.to(DEV).requires_grad_(True), y.to(DEV)
    out = photometric_loss(img, gt, lam)
    res = {"loss": out.loss, "l1": out.l1, "ssim": out.ssim, "psnr": out.psnr,
           "ssim_image": photometric.ssim(img, gt, size_average=False), "psnr_chw": photometric.psnr(img[0], gt[0])}
    res["grad"], = torch.autograd.grad(out.loss, img, retain_graph=True)
    res["grad_l1"], = torch.autograd.grad(out.l1, img, retain_graph=True)
    res["grad_ssim"], = torch.autograd.grad(out.ssim, img)
    return {k: v.detach() for k, v in res.items()}


_RATIOS = {}


def _record(case_id, entry):
    _RATIOS[case_id] = entry
    if not os.environ.get("HGS_WRITE_PROFILES"):
        return
    doc = {"what": "per case of tests/test_gpu_photometric.py and per quantity: [distance of the kernels from the float64 run of "
                   "the formulas, distance of the float32 CPU run of the formulas from it, gate = max(4 x the second, floor)]; "
                   "scalars: |v - v64| / max(1, |v64|), floor 1e-6; gradients: max |g - g64| / max(max |g64|, 1 / numel), floor "
                   "1e-5; ratio_to_reference: the worst first / second over the quantities whose second is not 0",
           "device": torch.cuda.get_device_name(0), "cases": dict(sorted(_RATIOS.items()))}
    with open(os.path.join(ROOT, "profiles", "photometric_parity.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _check(case_id, kind, B, C, H, W, seed=0):
    x, y, r64, r32, gates = _reference(kind, B, C, H, W, seed)
    got = _run_hip(x, y)
    assert got["psnr"].shape == (B, 1) and got["psnr_chw"].shape == (C, 1) and got["ssim_image"].shape == (B,)
    assert got["loss"].dim() == 0 and got["l1"].dim() == 0 and got["ssim"].dim() == 0 and got["grad"].shape == x.shape
    entry, failed, ratios = {}, [], []
    for k, gate in gates.items():
        dist = PR.grad_distance if k.startswith("grad") else PR.scalar_distance
        d, ref = dist(got[k], r64[k]), dist(r32[k], r64[k])
        entry[k] = [d, ref, gate]
        if ref > 0:
            ratios.append(d / ref)
        if not d <= gate:
            failed.append((k, d, ref, gate))
    entry["ratio_to_reference"] = max(ratios) if ratios else 0.0
    print(case_id, entry)
    _record(case_id, entry)
    assert not failed, (case_id, failed)
    return got, r64


@pytest.mark.parametrize("planes", PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_size_sweep(size, planes):
    (H, W), (B, C) = size, planes
    _check(f"sweep_{B}x{C}x{H}x{W}", "random", B, C, H, W, seed=H * 131 + W)


@pytest.mark.parametrize("kind", PR.CONTENT_KINDS)
def test_content_cases(kind):
    got, r64 = _check(f"content_{kind}", kind, 1, 3, 37, 53, seed=11)
    if kind == "constant_equal":
        assert float(got["loss"]) == 0.0 and float(got["l1"]) == 0.0 and float(got["ssim"]) == 1.0
        assert bool((got["grad_l1"] == 0).all()), "sign(0) must be 0"
        assert bool(torch.isinf(got["psnr"]).all() and (got["psnr"] > 0).all() and torch.isinf(got["psnr_chw"]).all())
        assert bool(torch.isinf(r64["psnr"]).all())
    if kind == "half_equal":
        x, y = _reference(kind, 1, 3, 37, 53, 11)[:2]
        same = (x == y).to(DEV)
        assert 0.3 < float(same.float().mean()) < 0.7
        assert bool((got["grad_l1"][same] == 0).all()) and bool((got["grad_l1"][~same].abs() > 0).all())
    if kind == "one_vs_zero":
        assert float(got["l1"]) == 1.0 and bool((got["psnr"] == 0).all())


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_reduction_boundaries(name):
    B, C, H, W = BOUNDARIES[name]
    tiles = -(-H // TH) * -(-W // TW)
    if name.startswith("tiles_"):
        assert tiles == int(name.split("_")[1])
    _check(f"boundary_{name}", "random", B, C, H, W, seed=5)


def test_two_calls_are_bit_identical_and_a_batch_equals_its_images():
    B, C, H, W = 2, 3, 45, 70
    x, y = PR.content_case("random", B, C, H, W, seed=21)
    a, b = _run_hip(x, y), _run_hip(x, y)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for i in range(B):
        one = _run_hip(x[i:i + 1], y[i:i + 1])
        assert torch.equal(one["ssim_image"], a["ssim_image"][i:i + 1])
        assert torch.equal(one["psnr"], a["psnr"][i:i + 1])
        for k in ("grad", "grad_l1", "grad_ssim"):      # the batch's means divide by B = 2 more: an exact scaling
            assert torch.equal(one[k], a[k][i:i + 1] * B), (k, i)


def test_autograd_plumbing():
    x, y = PR.content_case("random", 2, 3, 20, 41, seed=31)
    lam = 0.2
    img, gt = x.to(DEV).requires_grad_(True), y.to(DEV)

    def grad_of(pick, lam_):
        return torch.autograd.grad(pick(photometric_loss(img, gt, lam_)), img)[0]
    # a loss on l1 alone / ssim alone == the combined loss with the other weight at zero
    assert torch.equal(grad_of(lambda o: o.l1, lam), grad_of(lambda o: o.loss, 0.0))
    assert torch.equal(grad_of(lambda o: -o.ssim, lam), grad_of(lambda o: o.loss, 1.0))
    assert torch.equal(grad_of(lambda o: o.l1, lam), torch.autograd.grad(photometric.l1_loss(img, gt), img)[0])
    assert torch.equal(grad_of(lambda o: o.ssim, lam), torch.autograd.grad(photometric.ssim(img, gt), img)[0])
    per_image = torch.autograd.grad(photometric.ssim(img, gt, size_average=False).sum(), img)[0]
    r64 = PR.run(x, y, torch.float64)
    assert PR.grad_distance(per_image, r64["grad_ssim"] * 2) <= 1e-5       # sum over B = 2 images of per-image means
    # an unused output arrives as None, not as zeros
    seen = {}
    orig = photometric._Photometric.backward

    def spy(ctx, *grads):
        seen["grads"] = grads
        return orig(ctx, *grads)
    photometric._Photometric.backward = staticmethod(spy)
    try:
        photometric_loss(img, gt, lam).l1.backward()
    finally:
        photometric._Photometric.backward = staticmethod(orig)
    g = seen["grads"]
    assert g[1] is not None and g[0] is None and g[2] is None and g[3] is None
    assert not photometric_loss(img, gt).psnr.requires_grad and photometric_loss(img, gt).loss.requires_grad
    # gt receives nothing and says so
    with pytest.raises(ValueError, match="requires grad"):
        photometric_loss(img, gt.clone().requires_grad_(True))


def test_metrics_only_mode_allocates_no_derivative_maps():
    lib = _lib.load()
    B, C, H, W = 2, 3, 256, 256
    maps = 3 * B * C * H * W * 4
    small, full = lib.hgs_photometric_workspace_bytes(B, C, H, W, 0), lib.hgs_photometric_workspace_bytes(B, C, H, W, 1)
    assert full - small == maps and small < maps // 64
    assert lib.hgs_photometric_workspace_bytes(B, C, H, 40000, 0) == 0 and lib.hgs_photometric_workspace_bytes(70000, 1, 1, 1, 0) == 0
    x, y = PR.content_case("random", B, C, H, W, seed=2)
    img, gt = x.to(DEV).requires_grad_(True), y.to(DEV)
    with torch.no_grad():
        photometric_loss(img, gt)                                         # warm: the library and the allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        quiet = photometric_loss(img, gt)
        torch.cuda.synchronize()
        peak_quiet = torch.cuda.max_memory_allocated() - base
    assert not quiet.loss.requires_grad
    assert peak_quiet < maps // 8, (peak_quiet, maps)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loud = photometric_loss(img, gt)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base >= maps
    assert torch.equal(loud.loss.detach(), quiet.loss) and torch.equal(loud.psnr, quiet.psnr)
    # the raw ABI: a NULL argument block or pointer is refused before any device work
    assert lib.hgs_photometric_forward(None, None) != 0 and lib.hgs_photometric_backward(None, None) != 0
    args = _lib.HgsPhotometricArgs(B=1, C=1, H=4, W=4)
    assert lib.hgs_photometric_forward(ctypes.byref(args), None) != 0


def test_casts_non_contiguous_fp16_and_3d_inputs():
    x, y = PR.content_case("random", 1, 3, 37, 53, seed=41)
    want = _run_hip(x, y)
    # a non-contiguous view of the same values
    wide = torch.zeros(1, 3, 37, 106)
    wide[..., ::2] = x
    img = wide.to(DEV)[..., ::2].requires_grad_(True)
    assert not img.is_contiguous()
    out = photometric_loss(img, y.to(DEV))
    assert torch.equal(out.loss.detach(), want["loss"])
    assert torch.equal(torch.autograd.grad(out.loss, img)[0], want["grad"])
    # (C, H, W): the same numbers, psnr per channel
    img3 = x[0].to(DEV).requires_grad_(True)
    out3 = photometric_loss(img3, y[0].to(DEV))
    assert torch.equal(out3.loss.detach(), want["loss"]) and torch.equal(out3.psnr, want["psnr_chw"])
    g3, = torch.autograd.grad(out3.loss, img3)
    assert g3.shape == (3, 37, 53) and torch.equal(g3, want["grad"][0])
    # fp16 inputs are cast to fp32 once; the gradient comes back in the input's dtype
    xh, yh = x.half(), y.half()
    imgh = xh.to(DEV).requires_grad_(True)
    outh = photometric_loss(imgh, yh.to(DEV))
    ref = _run_hip(xh.float(), yh.float())
    assert outh.loss.dtype == torch.float32 and torch.equal(outh.loss.detach(), ref["loss"])
    gh, = torch.autograd.grad(outh.loss, imgh)
    assert gh.dtype == torch.float16 and torch.equal(gh, ref["grad"].half())


def test_end_to_end_through_render():
    """2000 Gaussians, one 64 x 64 view, gt = the render perturbed: the parameter gradients of photometric_loss(render, gt)
    against the rasterizer's backward fed with the float64 image gradient of the formulas (the truth) - the float32
    torch-op formulas on the GPU through the same render are the yardstick, margin 4, floor 1e-5 of max |gradient|."""
    from humangaussian_amd import synth
    from humangaussian_amd.renderer import render
    from test_gpu_api_contract import FakeCamera, FakeGaussianModel, Pipe
    cl = synth.init_cloud(2000, 1, "mid", seed=5, source="capsule")
    sc = {"means3D": cl.means3D, "shs": cl.shs, "opacities": cl.opacities, "scales": cl.scales, "rotations": cl.rotations}
    cam = FakeCamera(synth.orbit_camera(10.0, 30.0, 2.0, 50.0, 64, 64))
    bg = torch.zeros(3, device=DEV)
    state = {}

    def param_grads(image_grad):
        pc = FakeGaussianModel(sc, 1)
        image = render(cam, pc, Pipe(), bg)["render"]
        if "gt" not in state:
            noise = torch.randn(image.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
            state["gt"] = (image.detach() + 0.05 * noise).clamp(0.0, 1.0)
        image_grad(image, state["gt"])
        return [p.grad.detach().double().cpu() for p in pc.params()]

    def via_hip(image, gt):
        photometric_loss(image, gt).loss.backward()

    def via_torch_ops(image, gt):
        PR.formulas(image, gt)["loss"].backward()

    def via_fp64(image, gt):
        g = PR.run(image.detach().cpu(), gt.cpu(), torch.float64)["grad"]
        image.backward(g.float().to(DEV))

    truth, yard, got = param_grads(via_fp64), param_grads(via_torch_ops), param_grads(via_hip)
    assert float(state["gt"].std()) > 0.01
    entry, failed = {}, []
    for name, t, r, g in zip(("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"), truth, yard, got):
        assert bool(torch.isfinite(g).all()) and float(t.abs().max()) > 0
        scale = float(t.abs().max())
        d, ref = float((g - t).abs().max()) / scale, float((r - t).abs().max()) / scale
        gate = max(PR.MARGIN * ref, PR.GRAD_FLOOR)
        entry[name] = [d, ref, gate]
        if not d <= gate:
            failed.append((name, d, ref, gate))
    print("end_to_end", entry)
    _record("end_to_end", entry)
    assert not failed, failed
