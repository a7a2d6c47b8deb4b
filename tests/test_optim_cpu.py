"""CPU tests of the fused Adam step's host side (no GPU): the C ABI's new symbol in header, ctypes table and torch
binding; `GaussianAdam` as `torch.optim.Adam` on CPU tensors; the numpy restatement the GPU tests compare the kernel with;
the `prune_only` fixture."""
import copy
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import adam_reference as ar
from humangaussian_amd import _lib
from humangaussian_amd.optim import GaussianAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"))


def reference_groups(P, deg, seed):
    g = torch.Generator().manual_seed(seed)
    return [{"params": [torch.nn.Parameter(torch.randn(shape, generator=g))], "lr": ar.REFERENCE_LRS[name], "name": name}
            for name, shape in ar.reference_shapes(P, deg).items()]


def set_grads(groups, gen, scale=0.1):
    for grp in groups:
        p = grp["params"][0]
        p.grad = torch.randn(p.shape, generator=gen) * scale


def test_header_exports_and_binding_agree_on_adam_step():
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    assert re.search(r"^int hgs_adam_step\(const hgs_adam_args\* args, void\* stream\);", hdr, flags=re.M)
    assert int(re.search(r"#define HGS_ADAM_MAX_TENSORS (\d+)", hdr).group(1)) == _lib.ADAM_MAX_TENSORS == 16
    assert "hgs_adam_step" in _lib.EXPORTS
    _lib.build()
    lib = _lib.load()
    assert lib.hgs_abi_version() == 17 == _lib.ABI_VERSION
    # the struct of the header, field for field (natural LP64 layout: 4 pointers, int64, int32 + 6 floats, padded to 8)
    fields = re.search(r"typedef struct hgs_adam_tensor \{(.*?)\} hgs_adam_tensor;", hdr, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in _lib.HgsAdamTensor._fields_]
    assert ctypes.sizeof(_lib.HgsAdamTensor) == 72 and _lib.HgsAdamTensor.step_size.offset == 44
    assert ctypes.sizeof(_lib.HgsAdamArgs) == 24 + 16 * 72 + 17 * 4 + 4 and _lib.HgsAdamArgs.t.offset == 24
    # argument validation needs no GPU: nothing is launched
    a = _lib.HgsAdamArgs()
    assert lib.hgs_adam_step(None, None) == -1
    assert lib.hgs_adam_step(ctypes.byref(a), None) == 0                 # zero tensors
    a.num_tensors = 17
    assert lib.hgs_adam_step(ctypes.byref(a), None) == -1
    a.num_tensors = 2
    a.t[0].rows, a.t[0].row_floats = 0, 3
    a.t[1].rows, a.t[1].row_floats = 7, 0
    assert lib.hgs_adam_step(ctypes.byref(a), None) == 0                 # zero elements
    a.t[1].row_floats = 2
    assert lib.hgs_adam_step(ctypes.byref(a), None) == -1                # elements but null pointers
    a.t[1].rows = -1
    assert lib.hgs_adam_step(ctypes.byref(a), None) == -1
    a.t[1].rows, a.t[1].row_floats = 7, 0
    a.visible, a.visible_rows = 256, 7
    assert lib.hgs_adam_step(ctypes.byref(a), None) == -2                # tensor 0 has 0 rows, the mask 7
    _lib.build_binding()
    doc = _lib.load_binding().adam_step.__doc__
    for arg in ("params", "grads", "exp_avgs", "exp_avg_sqs", "scalars", "visible"):
        assert arg in doc
    with pytest.raises(RuntimeError, match="HIP device"):
        z = torch.zeros(3)
        _lib.load_binding().adam_step([z], [z], [z], [z], [[1.0] * 6])


def test_gaussian_adam_on_cpu_is_torch_adam_bit_for_bit():
    """the reference's six groups, its learning rates and eps=1e-15, five steps, the xyz rate rescheduled on the way"""
    ga, gb = reference_groups(40, 3, 1), reference_groups(40, 3, 1)
    a = torch.optim.Adam(ga, lr=0.0, eps=1e-15)
    b = GaussianAdam(gb, lr=0.0, eps=1e-15)
    assert isinstance(b, torch.optim.Adam) and not getattr(b, "_step_supports_amp_scaling", False)
    gen_a, gen_b = torch.Generator().manual_seed(2), torch.Generator().manual_seed(2)
    for it in range(5):
        set_grads(ga, gen_a)
        set_grads(gb, gen_b)
        for opt in (a, b):
            opt.param_groups[0]["lr"] = 1.6e-4 * 0.9 ** it
        a.step()
        b.step()
    for x, y in zip(ga, gb):
        px, py = x["params"][0], y["params"][0]
        assert torch.equal(px, py), x["name"]
        sx, sy = a.state[px], b.state[py]
        assert sorted(sx) == sorted(sy) == ["exp_avg", "exp_avg_sq", "step"]
        assert sy["step"].device.type == "cpu" and sy["step"].dtype == sx["step"].dtype and float(sy["step"]) == 5.0
        assert torch.equal(sx["exp_avg"], sy["exp_avg"]) and torch.equal(sx["exp_avg_sq"], sy["exp_avg_sq"])
    # a parameter without a gradient is skipped (no state appears), as torch skips it
    extra = torch.nn.Parameter(torch.ones(3))
    b.add_param_group({"params": [extra], "lr": 0.1, "name": "extra"})
    b.step()
    assert extra not in b.state and torch.equal(extra.detach(), torch.ones(3))


def test_fp32_restatement_within_the_p_bound_of_torch_cpu_adam():
    """One step at a time from torch's own state (the bound is a bound per step): the parameter within
    2^-21 |u| + ulp(p) of torch's CPU Adam over five steps of all six groups.  Torch orders two products differently
    ((w2 g) g, and it may fuse the moment update), so its moments are not asked to be bit-equal here."""
    groups = reference_groups(64, 3, 3)
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(4)
    worst = 0.0
    for t in range(1, 6):
        set_grads(groups, gen)
        before = []
        for grp in groups:
            p = grp["params"][0]
            st = opt.state.get(p, {})
            before.append((p.detach().numpy().copy(), p.grad.numpy().copy(),
                           st["exp_avg"].numpy().copy() if st else np.zeros(p.shape, np.float32),
                           st["exp_avg_sq"].numpy().copy() if st else np.zeros(p.shape, np.float32)))
        opt.step()
        for grp, (p0, g, m0, v0) in zip(groups, before):
            p1, m1, v1, u = ar.step_fp32(p0, g, m0, v0, grp["lr"], 0.9, 0.999, 1e-15, t)
            got = grp["params"][0].detach().numpy()
            err = np.abs(got.astype(np.float64) - p1.astype(np.float64))
            bound = ar.p_bound(u, p1)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (grp["name"], t, float((err / bound).max()))
            st = opt.state[grp["params"][0]]
            # (moments: a few roundings of their operands apart - the sum may cancel, so relative to the operands)
            eps32 = 2.0 ** -24
            assert (np.abs(st["exp_avg"].numpy() - m1) <= 4 * eps32 * (np.abs(m0) + np.abs(g))).all()
            assert (np.abs(st["exp_avg_sq"].numpy() - v1) <= 4 * eps32 * (v0 + g * g)).all()
    print("worst err / bound:", worst)
    # and the fp64 restatement is the same function: fp32 within a few ulp of it after one step
    p0, g, m0, v0 = before[0]
    p64, m64, v64 = ar.step_fp64(p0, g, m0, v0, 1.6e-4, 0.9, 0.999, 1e-15, 5)
    p32, m32, v32, _ = ar.step_fp32(p0, g, m0, v0, 1.6e-4, 0.9, 0.999, 1e-15, 5)
    assert np.abs(p32 - p64).max() <= 2 * ar.ulp(p32).max() and np.allclose(m32, m64, rtol=1e-6) and np.allclose(v32, v64, rtol=1e-6)


def test_from_optimizer_preserves_groups_and_state():
    groups = reference_groups(16, 1, 5)
    a = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(6)
    set_grads(groups, gen)
    a.step()
    b = GaussianAdam.from_optimizer(a)
    assert [g["name"] for g in b.param_groups] == [n for n, _ in GROUPS]
    for ga, gb in zip(a.param_groups, b.param_groups):
        assert gb["params"][0] is ga["params"][0] and gb["lr"] == ga["lr"] and gb["eps"] == 1e-15 and gb["betas"] == ga["betas"]
        sa, sb = a.state[ga["params"][0]], b.state[gb["params"][0]]
        assert sb["exp_avg"] is sa["exp_avg"] and sb["exp_avg_sq"] is sa["exp_avg_sq"] and float(sb["step"]) == 1.0
    # the adopted optimizer continues where the other stood: the same second step as an uninterrupted torch.optim.Adam
    twin = reference_groups(16, 1, 5)
    c = torch.optim.Adam(twin, lr=0.0, eps=1e-15)
    gen2 = torch.Generator().manual_seed(6)
    set_grads(twin, gen2)
    c.step()
    set_grads(twin, gen2)
    c.step()
    set_grads(groups, gen)
    b.step()
    for x, y in zip(groups, twin):
        assert torch.equal(x["params"][0], y["params"][0])
    with pytest.raises(TypeError):
        GaussianAdam.from_optimizer(torch.optim.SGD([torch.nn.Parameter(torch.ones(1))], lr=0.1))
    with pytest.raises(ValueError):
        GaussianAdam.from_optimizer(torch.optim.Adam([torch.nn.Parameter(torch.ones(1))], amsgrad=True))


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True),
                                dict(fused=True), dict(weight_decay=0.01)], ids=lambda kw: next(iter(kw)))
def test_constructor_refusals(kw):
    p = torch.nn.Parameter(torch.ones(2))
    with pytest.raises(ValueError, match=next(iter(kw))):
        GaussianAdam([p], **kw)
    opt = GaussianAdam([p])
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))], **kw})
    assert len(opt.param_groups) == 1


def test_state_dict_round_trip():
    groups = reference_groups(16, 1, 7)
    a = GaussianAdam(groups, lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(8)
    for _ in range(2):
        set_grads(groups, gen)
        a.step()
    sd = a.state_dict()
    assert [g["name"] for g in sd["param_groups"]] == [n for n, _ in GROUPS]
    twin = [{"params": [torch.nn.Parameter(g["params"][0].detach().clone())], "lr": 123.0, "name": g["name"]} for g in groups]
    b = GaussianAdam(twin, lr=0.0, eps=1e-15)
    b.load_state_dict(copy.deepcopy(sd))      # (as after torch.save / torch.load: load_state_dict itself keeps the tensors it is given)
    t = torch.optim.Adam([{"params": [torch.nn.Parameter(g["params"][0].detach().clone())], "lr": 123.0, "name": g["name"]}
                          for g in groups], lr=0.0, eps=1e-15)
    t.load_state_dict(copy.deepcopy(sd))                                                     # and torch's own class reads the same dict
    for grp, tw in zip(a.param_groups, b.param_groups):                       # (load_state_dict installs new group dicts)
        sa, sb = a.state[grp["params"][0]], b.state[tw["params"][0]]
        assert tw["lr"] == grp["lr"] and float(sb["step"]) == 2.0 and sb["step"].device.type == "cpu"
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    g1, g2, g3 = (torch.Generator().manual_seed(9) for _ in range(3))
    set_grads(a.param_groups, g1)
    set_grads(b.param_groups, g2)
    set_grads(t.param_groups, g3)
    a.step()
    b.step()
    t.step()
    for grp, tw, tt in zip(a.param_groups, b.param_groups, t.param_groups):
        assert torch.equal(grp["params"][0], tw["params"][0]) and torch.equal(grp["params"][0], tt["params"][0])


def test_prune_only_fixture_reproduces():
    """tests/golden/reference_prune_only.npz: (1) is what the method's definition (gaussian_model.py:426-432, :301-315)
    gives in plain boolean indexing on the recorded inputs; (2) where the reference tree is at hand, is what the
    generator's `--check` reproduces from the reference's own class, bit for bit."""
    fx = np.load(os.path.join(GOLD, "reference_prune_only.npz"))
    min_opacity, size_thresh = (float(x) for x in fx["args"])
    opacity = torch.sigmoid(torch.from_numpy(fx["in_opacity"]))
    scaling = torch.exp(torch.from_numpy(fx["in_scaling"]))
    mask = torch.logical_or((opacity < min_opacity).squeeze(), scaling.max(dim=1).values > size_thresh).numpy()
    assert np.array_equal(mask, fx["prune_mask"]) and 100 < mask.sum() < mask.size - 100
    assert (opacity < min_opacity).sum() > 10                                  # both criteria decide rows
    for name, attr in GROUPS:
        for src, dst in (("in" + attr, "out" + attr), ("in_exp_avg_" + name, "out_exp_avg_" + name),
                         ("in_exp_avg_sq_" + name, "out_exp_avg_sq_" + name)):
            assert np.array_equal(fx[src][~mask], fx[dst]), dst
    for key in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert np.array_equal(fx["in_" + key][~mask], fx["out_" + key]), key
    assert np.abs(fx["in_exp_avg_xyz"]).max() > 0 and np.abs(fx["in_xyz_gradient_accum"]).max() > 0
    spec = importlib.util.spec_from_file_location("make_prune_only_fixture", os.path.join(GOLD, "make_prune_only_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if gen.available():
        gen.check()
