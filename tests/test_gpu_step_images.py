"""GPU tests of `guidance_images` (csrc/step_images.hip, humangaussian_amd/step_images.py).

What the kernels are held to (tests/step_images_reference.py): per tensor - the two images, the two losses and the two
input gradients - max |error| against the float64 run of the formulas <= 4 x the float32 CPU run's own max error on the
same case, with a floor of 16 eps32 max|value|.  The factor 4 is a margin for the kernels' different partition of the
sums (a thread's pixels in order, a fixed tree over a workgroup, the partials in fp64), not a measured bound.  A second
check of the same form leaves out the pixels that tie for an extremum: their shares are orders of magnitude above the
other gradients of the depth and would otherwise set the scale for all of them.  Exact where it can be derived: the
minima, maxima, an empty view's image, fp16 against fp32, run against run.  Shapes are the smallest that reach every
branch; the table is built from the kernels' chunk sizes.  HGS_WRITE_PROFILES=1 records the per-case ratios in
profiles/step_images_parity.json."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import step_images_reference as sr
from humangaussian_amd import _lib, guidance_images

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
CASES = sr.sweep_cases(_lib.SI_PIXELS_PER_THREAD, _lib.SI_PIXELS_PER_WORKGROUP, _lib.SI_PARTIALS_PER_VIEW)
CHECKED = ("rgb", "depth", "loss_sparsity", "loss_opaque", "grad_render", "grad_depth")


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    """inputs, incoming gradients and the two CPU runs of a case: computed once, shared, never modified"""
    case = next(c for c in CASES if c["id"] == case_id)
    render, depth = sr.make_inputs(case)
    grads = sr.make_grads(case)
    size = (case["h"], case["w"])
    return case, render, depth, grads, sr.run(render, depth, size, grads, torch.float64), sr.run(render, depth, size, grads, torch.float32)


def _run_hip(render, depth, size, grads, dtype=torch.float32, grad_dtype=None):
    r = render.to(DEV).requires_grad_(True)
    d = depth.to(DEV).requires_grad_(True)
    out = guidance_images(r, d, size=size, dtype=dtype)
    names = [n for n in sr.OUTPUTS if n in grads]
    gs = []
    for n in names:
        g = grads[n].to(DEV)
        if n in ("rgb", "depth"):
            g = g.to(grad_dtype or dtype)
        gs.append(g)
    torch.autograd.backward([getattr(out, n) for n in names], gs)
    return out, r.grad, d.grad


def _finite(*tensors):
    for t in tensors:
        if t is not None:
            assert bool(torch.isfinite(t).all()), "NaN or Inf in an output"


_RATIOS = {}


def _record(case_id, entry):
    _RATIOS[case_id] = entry
    if not os.environ.get("HGS_WRITE_PROFILES"):
        return
    doc = {"what": "per case of tests/test_gpu_step_images.py and per tensor: max |error| of guidance_images against the float64 "
                   "run of the formulas (hip) and the float32 CPU run's own (ref), both in units of eps32 max|value|, and the "
                   "gate max(4 ref, 16) the first is held to; grad_depth_no_ties: the same over the pixels that tie for no extremum",
           "device": torch.cuda.get_device_name(0), "cases": dict(sorted(_RATIOS.items()))}
    with open(os.path.join(ROOT, "profiles", "step_images_parity.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _gate(name, got, r64, r32, entry, mask=None):
    """max |got - r64| <= max(4 max |r32 - r64|, 16 eps32 max |r64|), over `mask` if given; returns the failure or None"""
    got, a, b = np.asarray(got, np.float64), np.asarray(r64), np.asarray(r32)
    if mask is not None:
        got, a, b = got[mask], a[mask], b[mask]
        if got.size == 0:
            return None
    unit = sr.EPS32 * max(float(np.abs(a).max()), 1e-300)
    err, ref = float(np.abs(got - a).max()), float(np.abs(b - a).max())
    gate = max(4.0 * ref, 16.0 * unit)
    entry[name] = {"hip_over_unit": err / unit, "ref_over_unit": ref / unit, "gate_over_unit": gate / unit}
    return None if err <= gate else (name, entry[name])


@pytest.mark.parametrize("case_id", [c["id"] for c in CASES])
def test_sweep_against_fp64(case_id):
    case, render, depth, grads, r64, r32 = _reference(case_id)
    out, g_render, g_depth = _run_hip(render, depth, (case["h"], case["w"]), grads)
    B, h, w = case["B"], case["h"], case["w"]
    assert out.rgb.shape == out.depth.shape == (B, 3, h, w) and out.rgb.dtype == torch.float32 and out.rgb.is_contiguous()
    assert out.loss_sparsity.shape == out.loss_opaque.shape == out.depth_global_max.shape == () and out.depth_min.shape == (B,)
    assert not (out.depth_min.requires_grad or out.depth_max.requires_grad or out.depth_global_max.requires_grad)
    _finite(*out, g_render, g_depth)
    # exact: min and max are selections; the three depth channels are one value; an empty view normalises to 0
    d_dev = depth.to(DEV)
    assert torch.equal(out.depth_min, torch.amin(d_dev, dim=[1, 2, 3])) and torch.equal(out.depth_max, torch.amax(d_dev, dim=[1, 2, 3]))
    assert torch.equal(out.depth_global_max, d_dev.max())
    assert torch.equal(out.depth[:, 0], out.depth[:, 1]) and torch.equal(out.depth[:, 0], out.depth[:, 2])
    for b in range(B):
        if float(depth[b].abs().max()) == 0.0:
            assert float(out.depth[b].detach().abs().max()) == 0.0
    # which input gradients exist
    assert (g_render is None) == (r64["grad_render"] is None) and (g_depth is None) == (r64["grad_depth"] is None)
    got = {"rgb": out.rgb, "depth": out.depth, "loss_sparsity": out.loss_sparsity, "loss_opaque": out.loss_opaque,
           "grad_render": g_render, "grad_depth": g_depth}
    entry, failed = {}, []
    for name in CHECKED:
        if got[name] is None:
            continue
        failed.append(_gate(name, got[name].detach().cpu().numpy(), r64[name], r32[name], entry))
    if g_depth is not None:
        dn = depth.numpy()
        ties = (dn == dn.min(axis=(1, 2, 3), keepdims=True)) | (dn == dn.max(axis=(1, 2, 3), keepdims=True)) | (dn == dn.max())
        failed.append(_gate("grad_depth_no_ties", g_depth.cpu().numpy(), r64["grad_depth"], r32["grad_depth"], entry, mask=~ties))
    print(case_id, entry)
    _record(case_id, entry)
    failed = [f for f in failed if f]
    assert not failed, (case_id, failed)


def _case(**want):
    return next(c["id"] for c in CASES if all(c[k] == v for k, v in want.items()))


REPEAT_CASES = [_case(tag="size", H=33), _case(tag="partials+1"), _case(content="empty_view", H=48, grads="all"),
                _case(tag="partials+1-ragged")]


@pytest.mark.parametrize("case_id", REPEAT_CASES)
def test_two_runs_are_bit_identical(case_id):
    case, render, depth, grads, _, _ = _reference(case_id)
    runs = [_run_hip(render, depth, (case["h"], case["w"]), grads) for _ in range(2)]
    (o1, r1, d1), (o2, r2, d2) = runs
    for a, b in list(zip(o1, o2)) + [(r1, r2), (d1, d2)]:
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _finite(*o1, r1, d1)


@pytest.mark.parametrize("case_id", [_case(tag="size", H=33), _case(tag="size", H=6), _case(content="empty_view", H=48, grads="all"),
                                     _case(tag="size", H=256, B=8)])
def test_fp16_images_are_the_rounded_fp32_images_and_fp16_gradients_are_their_values(case_id):
    case, render, depth, _, _, _ = _reference(case_id)
    grads = sr.make_grads(case, dtype=torch.float16)          # values fp16 can hold, kept as float32
    size = (case["h"], case["w"])
    o32, r32, d32 = _run_hip(render, depth, size, grads)
    o16, r16, d16 = _run_hip(render, depth, size, grads, dtype=torch.float16)
    assert o16.rgb.dtype == o16.depth.dtype == torch.float16 and o16.loss_sparsity.dtype == torch.float32
    assert torch.equal(o16.rgb, o32.rgb.half()) and torch.equal(o16.depth, o32.depth.half())
    for a, b in ((o16.loss_sparsity, o32.loss_sparsity), (o16.loss_opaque, o32.loss_opaque), (r16, r32), (d16, d32)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _finite(*o16, r16, d16)


def test_non_contiguous_inputs_and_an_unused_output():
    case, render, depth, grads, r64, r32 = _reference(_case(tag="size", H=33))
    size = (case["h"], case["w"])
    r_nc = render.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # channels-last strides
    d_nc = torch.stack([depth.to(DEV), depth.to(DEV)], dim=-1)[..., 0]                  # every second element
    assert not r_nc.is_contiguous() and not d_nc.is_contiguous()
    a = guidance_images(r_nc, d_nc, size=size)
    b = guidance_images(render.to(DEV), depth.to(DEV), size=size)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the loss alone: the images' gradients are absent, render gets none
    r = render.to(DEV).requires_grad_(True)
    d = depth.to(DEV).requires_grad_(True)
    out = guidance_images(r, d, size=size)
    (out.loss_sparsity + 0.25 * out.loss_opaque).backward()
    assert r.grad is None and d.grad is not None
    _finite(d.grad)
    with pytest.raises(ValueError):
        guidance_images(r, d, size=(case["H"] + 1, case["w"]))


def test_end_to_end_through_render_views():
    """200 Gaussians, 3 views at 64 x 64 -> 32 x 32: the parameter gradients of a loss on the images and the two losses,
    through guidance_images, against the same loss written as torch ops.  The truth is the rasterizer's backward fed
    with the float64 CPU gradients of the formulas; the torch-op formulation in float32 on the GPU is the yardstick."""
    from helpers import make_scene
    from humangaussian_amd import synth
    from humangaussian_amd.renderer import render_views
    from test_gpu_api_contract import FakeCamera, FakeGaussianModel, Pipe
    B, P, H, W, h, w = 3, 200, 64, 64, 32, 32
    sc = make_scene(P=P, sh_degree=1, seed=77, H=H, W=W, spread=0.3)
    cams = [FakeCamera(synth.orbit_camera(10.0 * b - 10.0, 120.0 * b, 2.0, 50.0, H, W)) for b in range(B)]
    bg = torch.zeros(3, device=DEV)
    g = torch.Generator().manual_seed(3)
    w_rgb, w_d = torch.randn(B, 3, h, w, generator=g), torch.randn(B, 3, h, w, generator=g)
    grads = {"rgb": w_rgb, "depth": w_d, "loss_sparsity": torch.tensor(1.0), "loss_opaque": torch.tensor(0.25)}

    def param_grads(image_grads):
        """image_grads(render, depth) -> (dL/drender, dL/ddepth) on the device, both detached"""
        pc = FakeGaussianModel(sc, 1)
        out = render_views(cams, pc, Pipe(), bg)
        g_r, g_d = image_grads(out["render"].detach(), out["depth_3dgs"].detach())
        torch.autograd.backward([out["render"], out["depth_3dgs"]], [g_r, g_d])
        return [p.grad.detach().cpu().double().numpy() for p in pc.params()], out

    def via_hip(render, depth):
        _, g_r, g_d = _run_hip(render, depth, (h, w), grads)
        return g_r, g_d

    def via_torch_ops(render, depth):
        r, d = render.clone().requires_grad_(True), depth.clone().requires_grad_(True)
        o = sr.formulas(r, d, (h, w))
        torch.autograd.backward([o[n] for n in sr.OUTPUTS], [grads[n].to(DEV) for n in sr.OUTPUTS])
        return r.grad, d.grad

    def via_fp64(render, depth):
        res = sr.run(render, depth, (h, w), grads, torch.float64)
        return torch.from_numpy(res["grad_render"]).float().to(DEV), torch.from_numpy(res["grad_depth"]).float().to(DEV)

    truth, out = param_grads(via_fp64)
    assert float((out["depth_3dgs"] == 0).float().mean()) > 0.2 and float(out["depth_3dgs"].max()) > 0      # ties for the minimum
    yard, _ = param_grads(via_torch_ops)
    got, _ = param_grads(via_hip)
    entry, failed = {}, []
    for i, name in enumerate(("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity")):
        assert np.isfinite(got[i]).all()
        failed.append(_gate(name, got[i], truth[i], yard[i], entry))
    print("end_to_end", entry)
    _record("end_to_end", entry)
    failed = [f for f in failed if f]
    assert not failed, failed
