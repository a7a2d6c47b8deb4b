"""CPU tests of the step's guidance images and opacity losses (csrc/step_images.hip, humangaussian_amd/step_images.py):
the ABI surface and its refusals without a device, the Python errors, and the torch restatement the GPU tests compare
with (tests/step_images_reference.py) against the closed forms it must reproduce."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_images_reference as sr
from humangaussian_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPT, PPW, PPV = _lib.SI_PIXELS_PER_THREAD, _lib.SI_PIXELS_PER_WORKGROUP, _lib.SI_PARTIALS_PER_VIEW
CASES = sr.sweep_cases(PPT, PPW, PPV)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_header_declares_the_symbols_and_the_ctypes_mirror_matches():
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    assert re.search(r"^size_t hgs_step_images_workspace_bytes\(int32_t B, int32_t H, int32_t W, int32_t h, int32_t w\);", hdr, flags=re.M)
    assert re.search(r"^int hgs_step_images_forward\(const hgs_step_images_args\* args, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int hgs_step_images_backward\(const hgs_step_images_args\* args, void\* stream\);", hdr, flags=re.M)
    for name in ("hgs_step_images_workspace_bytes", "hgs_step_images_forward", "hgs_step_images_backward"):
        assert name in _lib.EXPORTS
    for name, val in (("PIXELS_PER_THREAD", PPT), ("PIXELS_PER_WORKGROUP", PPW), ("PARTIALS_PER_VIEW", PPV),
                      ("MAX_DIM", _lib.SI_MAX_DIM)):
        assert int(re.search(r"#define HGS_SI_%s (\d+)" % name, hdr).group(1)) == val
    fields = re.search(r"typedef struct hgs_step_images_args \{(.*?)\} hgs_step_images_args;", hdr, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in _lib.HgsStepImagesArgs._fields_]
    # six int32, then seventeen pointers
    assert _lib.HgsStepImagesArgs.render.offset == 24 and ctypes.sizeof(_lib.HgsStepImagesArgs) == 24 + 17 * 8
    assert _lib.ABI_VERSION == 17


def _args(**kw):
    """every pointer non-NULL and aligned (never dereferenced: each call below is refused before any device work)"""
    a = _lib.HgsStepImagesArgs()
    a.B, a.H, a.W, a.h, a.w = 2, 64, 48, 32, 24
    for name, _ in _lib.HgsStepImagesArgs._fields_[6:]:
        setattr(a, name, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_bad_arguments_return_minus_one_without_a_device(lib):
    EINVAL = -1
    for fn in (lib.hgs_step_images_forward, lib.hgs_step_images_backward):
        assert fn(None, None) == EINVAL
        for bad in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(h=-2), dict(h=65), dict(w=49),
                    dict(H=_lib.SI_MAX_DIM + 1, h=1), dict(B=65535, H=32768, W=32768)):
            assert fn(ctypes.byref(_args(**bad)), None) == EINVAL, bad
    for name in ("render", "depth", "workspace", "rgb_out", "depth_out", "loss_sparsity", "loss_opaque", "depth_min",
                 "depth_max", "depth_global_max", "tie_counts"):
        assert lib.hgs_step_images_forward(ctypes.byref(_args(**{name: None})), None) == EINVAL, name
    for name in ("render", "depth", "rgb_out", "depth_out", "workspace"):                      # 16-byte accesses
        assert lib.hgs_step_images_forward(ctypes.byref(_args(**{name: 4100})), None) == EINVAL, name
    for name in ("depth", "workspace", "depth_min", "depth_max", "depth_global_max", "tie_counts", "grad_depth_in", "grad_render"):
        assert lib.hgs_step_images_backward(ctypes.byref(_args(**{name: None})), None) == EINVAL, name
    # the flags: with grad_rgb alone nothing of the depth is needed, with the losses alone no grad_render
    none = dict(grad_rgb=None, grad_depth=None, grad_loss_sparsity=None, grad_loss_opaque=None)
    assert lib.hgs_step_images_backward(ctypes.byref(_args(**none)), None) == 0          # nothing to do: no launch
    assert lib.hgs_step_images_backward(ctypes.byref(_args(**none, B=0)), None) == EINVAL


def test_workspace_bytes_is_monotone_and_zero_for_bad_sizes(lib):
    ws = lib.hgs_step_images_workspace_bytes
    for bad in ((0, 8, 8, 4, 4), (1, 0, 8, 1, 4), (1, 8, 0, 4, 1), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0), (1, 8, 8, 9, 4), (1, 8, 8, 4, 9),
                (-1, 8, 8, 4, 4), (1, _lib.SI_MAX_DIM + 1, 8, 4, 4), (65535, 32768, 32768, 4, 4)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, 1, 1, 1) > 0 and ws(1, 1, 1, 1, 1) % 256 == 0
    base = (2, 300, 200, 100, 50)
    for i in range(5):
        prev = 0
        for v in (1, 2, 3, 7, 32, 50, 64, 100):
            s = list(base)
            s[i] = v
            if s[3] > s[1] or s[4] > s[2]:
                continue
            cur = ws(*s)
            assert cur >= prev > -1 and cur > 0, (i, v)
            prev = cur
    # the forward keeps seven words per partial; a view has at most PPV partials
    assert ws(8, 1024, 1024, 512, 512) >= 8 * PPV * 7 * 4
    assert ws(8, 1024, 1024, 512, 512) == ws(8, 2048, 2048, 512, 512)
    assert ws(3, 32, 32, 16, 16) >= (3 * 3 + 2 * 3 + 1) * 4


def test_python_errors():
    from humangaussian_amd import StepImages, guidance_images
    assert StepImages._fields == ("rgb", "depth", "loss_sparsity", "loss_opaque", "depth_min", "depth_max", "depth_global_max")
    r, d = torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        guidance_images(r, d, size=(4, 4))
    for bad_r, bad_d in ((r[0], d), (r, d[0]), (r[:, :2], d), (r, r), (r, d[:1]), (r, d[..., :4]), (r[:, :, :4], d)):
        with pytest.raises(ValueError):
            guidance_images(bad_r, bad_d, size=(4, 4))
    for size in ((9, 4), (4, 9), (0, 4), (4, 0), (512, 512), 4, (4,)):
        with pytest.raises(ValueError):
            guidance_images(r, d, size=size)
    with pytest.raises(ValueError):
        guidance_images(r, d, size=(4, 4), dtype=torch.bfloat16)
    _lib.build_binding()
    with pytest.raises(RuntimeError, match="HIP device"):
        _lib.load_binding().step_images_forward(r, d, 4, 4, False)


def test_two_to_one_resize_is_the_box_mean():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 12, 20, generator=g, dtype=torch.float64)
    d = torch.rand(2, 1, 12, 20, generator=g, dtype=torch.float64)
    out = sr.formulas(x, d, (6, 10))
    assert torch.equal(out["rgb"], F.avg_pool2d(x, 2))
    x32 = x.float()
    assert torch.equal(sr.formulas(x32, d.float(), (6, 10))["rgb"], F.avg_pool2d(x32, 2))


def test_tie_rule_and_bce_target_gradient_are_the_closed_forms():
    t = torch.tensor([1.0, 3.0, 3.0, 0.0], requires_grad=True)
    t.max().backward()
    assert t.grad.tolist() == [0.0, 0.5, 0.5, 0.0]
    t = torch.tensor([[1.0, 3.0, 3.0, 0.0], [0.0, 0.0, 2.0, 0.0]], requires_grad=True)
    (torch.amax(t, dim=[1]).sum() + 3.0 * torch.amin(t, dim=[1]).sum()).backward()
    assert t.grad.tolist() == [[0.0, 0.5, 0.5, 3.0], [1.0, 1.0, 1.0, 1.0]]
    x = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    F.binary_cross_entropy(x, x).backward()                    # the input's own part is (x - t) / (x (1 - x)) = 0
    assert abs(float(x.grad) - (np.log(0.7) - np.log(0.3))) < 1e-12 and abs(float(x.grad) - 0.8473) < 1e-4
    # through the formulas: a view whose every pixel ties, and the clamp that lets the BCE gradient through only inside
    d = torch.tensor([[[[0.0, 0.0], [0.0, 0.0]]], [[[0.5, 2.0], [2.0, 1e-4]]]], dtype=torch.float64, requires_grad=True)
    r = torch.zeros(2, 3, 2, 2, dtype=torch.float64)
    out = sr.formulas(r, d, (1, 1))
    assert float(out["depth"][0].detach().abs().max()) == 0.0
    out["loss_opaque"].backward()
    s = 2.0 + 1e-5
    inside = (np.log(1 - 0.5 / s) - np.log(0.5 / s)) / 8 / s
    got = d.grad[1, 0]
    assert abs(float(got[0, 0]) - inside) < 1e-12
    assert float(d.grad[0].abs().max()) == 0.0 and float(got[1, 1]) == 0.0       # op < 1e-3: clamped
    # the two maxima are clamped above; they share dL/dg = -sum(dL/dop op) / s
    share = -(inside * s) * (0.5 / s) / s / 2
    assert abs(float(got[0, 1]) - share) < 1e-12 and float(got[0, 1]) == float(got[1, 0])


def test_reference_gradient_matches_central_differences():
    g = torch.Generator().manual_seed(5)
    B, H, W, h, w = 2, 6, 5, 3, 4
    render = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64)
    depth = (0.3 + (torch.randperm(B * H * W, generator=g).double() + 0.5) / (B * H * W)).reshape(B, 1, H, W)   # tie-free
    w_rgb, w_d = torch.randn(B, 3, h, w, generator=g, dtype=torch.float64), torch.randn(B, 3, h, w, generator=g, dtype=torch.float64)

    def loss(r, d):
        o = sr.formulas(r, d, (h, w))
        return (o["rgb"] * w_rgb).sum() + (o["depth"] * w_d).sum() + o["loss_sparsity"] + 0.25 * o["loss_opaque"]
    r, d = render.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    loss(r, d).backward()
    eps = 1e-6
    for t, grad in ((render, r.grad), (depth, d.grad)):
        flat = t.reshape(-1)
        for i in range(flat.numel()):
            keep = float(flat[i])
            flat[i] = keep + eps
            up = float(loss(render, depth))
            flat[i] = keep - eps
            dn = float(loss(render, depth))
            flat[i] = keep
            fd = (up - dn) / (2 * eps)
            assert abs(fd - float(grad.reshape(-1)[i])) <= 1e-6 * max(1.0, abs(fd)), (i, fd, float(grad.reshape(-1)[i]))


def test_case_table_contains_every_boundary_it_claims():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    shapes = {((c["H"], c["W"]), (c["h"], c["w"])) for c in CASES}
    for HW, hw, B in sr.SIZES:
        assert any(c["tag"] == "size" and (c["H"], c["W"]) == HW and (c["h"], c["w"]) == hw and c["B"] == B for c in CASES)
    assert ((256, 256), (128, 128)) in shapes and any(c["B"] == 8 for c in CASES)
    by_tag = {c["tag"]: c for c in CASES}
    px = lambda tag: by_tag[tag]["H"] * by_tag[tag]["W"]  # noqa: E731
    assert px("thread") == PPT and px("thread+1") == PPT + 1
    assert px("chunk") == PPW and px("chunk+1") == PPW + 1
    assert sr.chunks_of(by_tag["partials"]["H"], by_tag["partials"]["W"], PPW) == PPV and px("partials") == PPV * PPW
    for tag in ("partials+1", "partials+1-ragged"):
        assert sr.chunks_of(by_tag[tag]["H"], by_tag[tag]["W"], PPW) == PPV + 1
    assert px("partials+1") % PPW == 0 and px("partials+1-ragged") % PPW != 0 and px("partials+1-ragged") % 4 != 0
    for c in CASES:
        assert 1 <= c["h"] <= c["H"] and 1 <= c["w"] <= c["W"] and 1 <= c["B"] <= 8
    assert {c["content"] for c in CASES} == set(sr.CONTENTS) and {c["grads"] for c in CASES} == set(sr.GRADS)
    # both forms of the 2:1 path (16-byte loads need W % 8 == 0) and the general gather
    two = [c for c in CASES if c["H"] == 2 * c["h"] and c["W"] == 2 * c["w"]]
    assert any(c["W"] % 8 == 0 for c in two) and any(c["W"] % 8 != 0 for c in two) and len(two) < len(CASES)
    # what the contents promise
    for c in CASES:
        if c["tag"] != "content" or (c["H"], c["W"]) != (33, 47):
            continue
        _, d = sr.make_inputs(c)
        k = c["content"]
        if k == "empty_view":
            assert float(d[c["B"] // 2].abs().max()) == 0.0 and all(float(d[b].max()) > 0 for b in range(c["B"]) if b != c["B"] // 2)
        elif k == "constant_view":
            assert float(d[c["B"] // 2].min()) == float(d[c["B"] // 2].max()) == 0.75
        elif k == "unique_min":
            assert float(d.min()) > 0 and d.unique().numel() == d.numel()
        elif k == "tie_max":
            assert int((d[0] == d[0].max()).sum()) == 2
        elif k == "tie_global":
            assert int((d == d.max()).sum()) == 2 and float(d[0].max()) == float(d[c["B"] - 1].max()) == float(d.max())
    blob = sr.make_inputs(next(c for c in CASES if c["tag"] == "partials"))[1]
    assert 0.6 <= float((blob == 0).float().mean()) <= 0.8


def test_fp32_reference_stays_finite_with_an_empty_view():
    c = next(c for c in CASES if c["content"] == "empty_view" and c["grads"] == "all" and c["H"] == 33)
    render, depth = sr.make_inputs(c)
    r32 = sr.run(render, depth, (c["h"], c["w"]), sr.make_grads(c), torch.float32)
    r64 = sr.run(render, depth, (c["h"], c["w"]), sr.make_grads(c), torch.float64)
    for k, v in r32.items():
        assert np.isfinite(v).all(), k
    assert float(np.abs(r32["depth"][c["B"] // 2]).max()) == 0.0
    big = float(np.abs(r64["grad_depth"]).max())
    assert big > 1e9 and float(np.abs(r32["grad_depth"] - r64["grad_depth"]).max()) <= 1e-5 * big
