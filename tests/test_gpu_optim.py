"""GPU tests of the fused Adam step (csrc/optim.hip, humangaussian_amd/optim.py) and of `densify.prune_only`.

What the kernel is held to (tests/adam_reference.py): after every step `exp_avg` and `exp_avg_sq` are BIT-EQUAL to the
fp32 restatement (adds and multiplies only, no contraction in this build) and `param` is within 2^-21 |u| + ulp(p) of
it (one square root and two divisions may differ in the last place, then one rounding of the sum).  Shapes are the
smallest at which this kernel can go wrong: element counts 0..3 mod 4, a tensor boundary inside a workgroup, more than
one workgroup per tensor, the 17th tensor of a call, an unaligned pointer, a zero-row tensor."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch

import adam_reference as ar
from humangaussian_amd import _lib, densify
from humangaussian_amd.optim import GaussianAdam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"))
BETAS, EPS = (0.9, 0.999), 1e-15


def dev():
    return torch.device("cuda")


def snapshot(opt, p):
    st = opt.state.get(p, {})
    zeros = np.zeros(tuple(p.shape), np.float32)
    return (p.detach().cpu().numpy().copy(), p.grad.cpu().numpy().copy(),
            st["exp_avg"].cpu().numpy().copy() if st else zeros, st["exp_avg_sq"].cpu().numpy().copy() if st else zeros)


def checked_step(opt, t, **kw):
    """One `opt.step(**kw)`, every parameter that has a gradient compared with the fp32 restatement of that step from the
    state the optimizer held before it.  Returns the worst err / bound of the parameters."""
    before = [(grp, p, snapshot(opt, p)) for grp in opt.param_groups for p in grp["params"] if p.grad is not None]
    opt.step(**kw)
    worst = 0.0
    for grp, p, (p0, g, m0, v0) in before:
        p1, m1, v1, u = ar.step_fp32(p0, g, m0, v0, grp["lr"], *grp["betas"], grp["eps"], t)
        st = opt.state[p]
        assert float(st["step"]) == t and st["step"].device.type == "cpu"
        assert np.array_equal(st["exp_avg"].cpu().numpy(), m1), ("exp_avg", tuple(p.shape), t)
        assert np.array_equal(st["exp_avg_sq"].cpu().numpy(), v1), ("exp_avg_sq", tuple(p.shape), t)
        if p.numel():
            err = np.abs(p.detach().cpu().numpy().astype(np.float64) - p1.astype(np.float64))
            bound = ar.p_bound(u, p1)
            print("shape", tuple(p.shape), "step", t, "max err / bound", float((err / bound).max()), "bit-equal", bool((err == 0).all()))
            assert (err <= bound).all(), (tuple(p.shape), t, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    return worst


def make_params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dev())) for s in shapes]


def give_grads(params, gen, scale=0.1):
    for p in params:
        p.grad = (torch.randn(tuple(p.shape), generator=gen) * scale).to(p.device)


@pytest.mark.parametrize("P", [1, 3, 5, 257, 1025])
def test_table_cases(P):
    """row_floats 1, 3, 4, 45 as four one-tensor groups with their own learning rates: ONE launch whose tensors end
    inside a workgroup's span, element counts on every residue mod 4; checked after each of five steps."""
    params = make_params([(P, rf) for rf in (1, 3, 4, 45)], seed=P)
    opt = GaussianAdam([{"params": [p], "lr": lr} for p, lr in zip(params, (1.6e-4, 0.0025, 0.05, 0.001))], lr=0.0, eps=EPS)
    gen = torch.Generator().manual_seed(100 + P)
    for t in range(1, 6):
        give_grads(params, gen)
        checked_step(opt, t)


def _reference_groups(P, deg, seed):
    g = torch.Generator().manual_seed(seed)
    vals = {name: torch.randn(shape, generator=g) for name, shape in ar.reference_shapes(P, deg).items()}
    return vals


def _grad_sequence(P, deg, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return [{name: torch.randn(shape, generator=g) * (0.1 if t % 3 else 0.02)
             for name, shape in ar.reference_shapes(P, deg).items()} for t in range(steps)]


def _run(cls, vals, grads, on):
    groups = [{"params": [torch.nn.Parameter(v.clone().to(on))], "lr": ar.REFERENCE_LRS[n], "name": n} for n, v in vals.items()]
    opt = cls(groups, lr=0.0, eps=EPS)
    for gs in grads:
        for grp in groups:
            grp["params"][0].grad = gs[grp["name"]].to(on)
        opt.step()
    return {grp["name"]: grp["params"][0].detach().cpu().numpy() for grp in opt.param_groups}, opt


_FP64 = {}


def _fp64_run(P, deg, steps):
    """the fp64 restatement over the prescribed gradients, computed once per (P, deg, steps) and left unchanged"""
    key = (P, deg, steps)
    if key not in _FP64:
        vals, grads = _reference_groups(P, deg, 11), _grad_sequence(P, deg, steps, 12)
        out = {}
        for n, v in vals.items():
            p, m, s = v.numpy().astype(np.float64), np.zeros(v.shape), np.zeros(v.shape)
            for t, gs in enumerate(grads, 1):
                p, m, s = ar.step_fp64(p, gs[n].numpy(), m, s, ar.REFERENCE_LRS[n], *BETAS, EPS, t)
            out[n] = p
        _FP64[key] = (vals, grads, out)
    return _FP64[key]


@pytest.mark.parametrize("deg", [0, 3])
def test_reference_groups_against_fp64_and_torch(deg):
    """The reference's six groups at P = 1000, 20 steps on a prescribed gradient sequence: GaussianAdam and the device's
    own torch.optim.Adam each against the fp64 restatement; per tensor the HIP distance (max-norm) may be at most twice
    torch's plus one ulp of the tensor's largest value (the two differ only in legitimate rounding order)."""
    P, steps = 1000, 20
    vals, grads, want = _fp64_run(P, deg, steps)
    hip, opt = _run(GaussianAdam, vals, grads, dev())
    tor, _ = _run(torch.optim.Adam, vals, grads, dev())
    assert all(float(opt.state[g["params"][0]]["step"]) == steps for g in opt.param_groups)
    pairs, bad = {}, []
    for n in vals:
        if want[n].size == 0:
            assert hip[n].size == 0
            continue
        d_hip, d_tor = float(np.abs(hip[n] - want[n]).max()), float(np.abs(tor[n] - want[n]).max())
        one = float(ar.ulp(np.float32(np.abs(want[n]).max())))
        pairs[n] = {"hip": d_hip, "torch": d_tor, "ulp_of_max": one, "moved": float(np.abs(want[n] - vals[n].numpy()).max())}
        print(n, pairs[n])
        if not d_hip <= 2 * d_tor + one:
            bad.append(n)
        assert pairs[n]["moved"] > 100 * one or ar.REFERENCE_LRS[n] < 1e-3, n       # the steps moved the tensor
    _record_parity(f"P{P}_sh{deg}", pairs)
    assert not bad, {n: pairs[n] for n in bad}


def _record_parity(key, pairs):
    path = os.path.join(ROOT, "profiles", "optim_parity.json")
    try:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.setdefault("what", "max-norm distance to the fp64 restatement after 20 steps, per tensor: GaussianAdam (hip) and "
                               "torch.optim.Adam on the same device (torch); tests/test_gpu_optim.py")
        doc["device"] = torch.cuda.get_device_name(0)
        doc[key] = pairs
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError as e:                      # a read-only checkout still runs the comparison
        print("not recorded:", e)


def test_seventeen_tensors_split_over_two_launches(monkeypatch):
    binding = _lib.load_binding()
    calls, real = [], binding.adam_step
    monkeypatch.setattr(binding, "adam_step", lambda *a: (calls.append(len(a[0])), real(*a))[1])
    params = make_params([(7 + i, 3) for i in range(17)], seed=17)
    opt = GaussianAdam(params, lr=0.01, eps=EPS)
    give_grads(params, torch.Generator().manual_seed(18))
    checked_step(opt, 1)
    assert calls == [17]                                    # one call of the binding, which splits at HGS_ADAM_MAX_TENSORS
    # the raw entry point refuses a 17th tensor rather than read past its table
    a = _lib.HgsAdamArgs()
    a.num_tensors = 17
    assert _lib.load().hgs_adam_step(a, None) == -1
    give_grads(params, torch.Generator().manual_seed(19))
    checked_step(opt, 2)


def test_skipped_and_empty_tensors():
    used, unused, empty = make_params([(33, 3), (33, 4), (0, 3)], seed=20)
    opt = GaussianAdam([{"params": [used]}, {"params": [unused]}, {"params": [empty]}], lr=0.01, eps=EPS)
    keep = unused.detach().clone()
    give_grads([used, empty], torch.Generator().manual_seed(21))
    checked_step(opt, 1)
    assert unused not in opt.state and torch.equal(unused.detach(), keep)
    assert float(opt.state[empty]["step"]) == 1.0 and opt.state[empty]["exp_avg"].shape == (0, 3)
    # only empty tensors: no launch at all, the step still counts
    lone = torch.nn.Parameter(torch.zeros(0, 4, device=dev()))
    o2 = GaussianAdam([lone], lr=0.01)
    lone.grad = torch.zeros(0, 4, device=dev())
    o2.step()
    assert float(o2.state[lone]["step"]) == 1.0
    torch.cuda.synchronize()


def test_misaligned_parameter_takes_the_scalar_form():
    P, rf = 1025, 3
    g = torch.Generator().manual_seed(22)
    base = torch.randn(P * rf + 1, generator=g).to(dev())
    odd = torch.nn.Parameter(base[1:].view(P, rf))                       # a leaf whose data starts 4 bytes into its storage
    assert odd.is_leaf and odd.is_contiguous() and odd.data_ptr() % 16 == 4
    even = torch.nn.Parameter(base[1:].view(P, rf).clone())
    assert even.data_ptr() % 16 == 0
    oa, ob = GaussianAdam([odd], lr=0.01, eps=EPS), GaussianAdam([even], lr=0.01, eps=EPS)
    gen = torch.Generator().manual_seed(23)
    for t in range(1, 4):
        give_grads([odd], gen)
        even.grad = odd.grad.clone()
        checked_step(oa, t)
        ob.step()
        assert torch.equal(odd.detach(), even.detach())
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[odd][k], ob.state[even][k])
    assert float(base[0]) == float(torch.randn(P * rf + 1, generator=torch.Generator().manual_seed(22))[0])   # the float in front is untouched


@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.uint8])
def test_visibility(mask_dtype):
    P = 257
    shapes = [(P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 4)]
    a, b = make_params(shapes, seed=24), make_params(shapes, seed=24)
    oa, ob = GaussianAdam(a, lr=0.01, eps=EPS), GaussianAdam(b, lr=0.01, eps=EPS)
    gen_a, gen_b = torch.Generator().manual_seed(25), torch.Generator().manual_seed(25)
    give_grads(a, gen_a)
    give_grads(b, gen_b)
    oa.step()
    ob.step()                                                            # live moments on both
    mask = (torch.rand(P, generator=torch.Generator().manual_seed(26)) < 0.4)
    assert 50 < int(mask.sum()) < P - 50
    vis = mask.to(dev()).to(mask_dtype)
    before = [(p.detach().clone(), oa.state[p]["exp_avg"].clone(), oa.state[p]["exp_avg_sq"].clone()) for p in a]
    give_grads(a, gen_a)
    give_grads(b, gen_b)
    with pytest.raises(ValueError, match="visibility"):
        oa.step(visibility=vis[:-1])
    with pytest.raises(ValueError, match="visibility"):
        oa.step(visibility=mask.to(dev()).float())
    assert all(float(oa.state[p]["step"]) == 1.0 for p in a)             # a refused call changed nothing
    oa.step(visibility=vis)
    ob.step()
    m = mask.to(dev())
    for p, q, (p0, m0, v0) in zip(a, b, before):
        got = (p.detach(), oa.state[p]["exp_avg"], oa.state[p]["exp_avg_sq"])
        dense = (q.detach(), ob.state[q]["exp_avg"], ob.state[q]["exp_avg_sq"])
        for x, x0, xd in zip(got, (p0, m0, v0), dense):
            assert torch.equal(x[~m].view(torch.int32), x0[~m].view(torch.int32))      # masked out: the bits stay
            assert torch.equal(x[m].view(torch.int32), xd[m].view(torch.int32))        # masked in: the dense step
            assert not torch.equal(x[m], x0[m])
        assert float(oa.state[p]["step"]) == 2.0                          # the count is global
    # the raw binding refuses a mask of the wrong length as well
    z = torch.zeros(4, 3, device=dev())
    with pytest.raises(RuntimeError, match="visible"):
        _lib.load_binding().adam_step([z], [z.clone()], [z.clone()], [z.clone()], [[1e-3, 1.0, 0.1, 0.999, 0.001, 1e-8]],
                                      torch.ones(5, dtype=torch.uint8, device=dev()))


def test_interchangeable_with_torch_adam():
    """three HIP steps, two torch steps from the same state, load_state_dict into a fresh GaussianAdam, one more HIP step:
    after every step within the accumulated per-step bound of an uninterrupted GaussianAdam run."""
    P, deg, steps = 300, 1, 6
    vals, grads = _reference_groups(P, deg, 31), _grad_sequence(P, deg, steps, 32)

    def groups_of(vs):
        return [{"params": [torch.nn.Parameter(v.clone().to(dev()))], "lr": ar.REFERENCE_LRS[n], "name": n} for n, v in vs.items()]

    def feed(opt, t):
        for grp in opt.param_groups:
            grp["params"][0].grad = grads[t][grp["name"]].to(dev())

    straight = GaussianAdam(groups_of(vals), lr=0.0, eps=EPS)
    mixed = GaussianAdam(groups_of(vals), lr=0.0, eps=EPS)
    allowed = {n: 0.0 for n in vals}
    for t in range(steps):
        if t == 3:      # torch's own class continues from the state (as after a save / load)
            sd = copy.deepcopy(mixed.state_dict())
            mixed = torch.optim.Adam([{"params": g["params"], "lr": 9.0, "name": g["name"]} for g in mixed.param_groups], lr=0.0, eps=EPS)
            mixed.load_state_dict(sd)
        if t == 5:
            sd = copy.deepcopy(mixed.state_dict())
            mixed = GaussianAdam([{"params": g["params"], "lr": 9.0, "name": g["name"]} for g in mixed.param_groups], lr=0.0, eps=EPS)
            mixed.load_state_dict(sd)
            assert type(mixed) is GaussianAdam
        feed(straight, t)
        feed(mixed, t)
        snaps = {g["name"]: snapshot(straight, g["params"][0]) for g in straight.param_groups}
        straight.step()
        mixed.step()
        for gs, gm in zip(straight.param_groups, mixed.param_groups):
            n = gs["name"]
            assert gm["lr"] == gs["lr"] and float(mixed.state[gm["params"][0]]["step"]) == t + 1
            p0, g, m0, v0 = snaps[n]
            p1, _, _, u = ar.step_fp32(p0, g, m0, v0, gs["lr"], *BETAS, EPS, t + 1)
            allowed[n] = allowed[n] + ar.p_bound(u, p1)
            err = np.abs(gs["params"][0].detach().cpu().numpy().astype(np.float64) - gm["params"][0].detach().cpu().numpy())
            print(n, "step", t + 1, "max err / allowed", float((err / allowed[n]).max()))
            assert (err <= allowed[n]).all(), (n, t + 1, float((err / allowed[n]).max()))
            if t < 3:
                assert (err == 0).all()


def _model_from(fx, optimizer_cls):
    pc = types.SimpleNamespace()
    plist = []
    for name, attr in GROUPS:
        p = torch.nn.Parameter(torch.from_numpy(fx["in" + attr]).to(dev()))
        setattr(pc, attr, p)
        plist.append({"params": [p], "lr": ar.REFERENCE_LRS[name], "name": name})
    pc.optimizer = optimizer_cls(plist, lr=0.0, eps=EPS)
    for name, attr in GROUPS:
        pc.optimizer.state[getattr(pc, attr)] = {"step": torch.tensor(3.0),
                                                 "exp_avg": torch.from_numpy(fx["in_exp_avg_" + name]).to(dev()),
                                                 "exp_avg_sq": torch.from_numpy(fx["in_exp_avg_sq_" + name]).to(dev())}
    pc.xyz_gradient_accum = torch.from_numpy(fx["in_xyz_gradient_accum"]).to(dev())
    pc.denom = torch.from_numpy(fx["in_denom"]).to(dev())
    pc.max_radii2D = torch.from_numpy(fx["in_max_radii2D"]).to(dev())
    return pc


def _compare_model(pc, fx, exact=False):
    for name, attr in GROUPS:
        p = getattr(pc, attr)
        group = next(g for g in pc.optimizer.param_groups if g["name"] == name)
        assert group["params"][0] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        st = pc.optimizer.state[p]
        assert len(pc.optimizer.state) == 6 and float(st["step"]) == 3.0
        for got, key in ((p.detach(), "out" + attr), (st["exp_avg"], "out_exp_avg_" + name), (st["exp_avg_sq"], "out_exp_avg_sq_" + name)):
            want = torch.from_numpy(fx[key])
            assert got.shape == want.shape, (key, got.shape, want.shape)
            err = float((got.cpu() - want).abs().max()) if want.numel() else 0.0
            assert err <= 1e-6 * max(1.0, float(want.abs().max())), (key, err)
            if exact:
                assert torch.equal(got.cpu(), want), key


def _one_more_step(pc, t):
    n = pc._xyz.shape[0]
    gen = torch.Generator().manual_seed(40)
    params = [getattr(pc, attr) for _, attr in GROUPS]
    assert all(p.shape[0] == n for p in params)
    give_grads(params, gen)
    checked_step(pc.optimizer, t)


def test_densify_and_prune_on_a_gaussian_adam():
    fx = np.load(os.path.join(GOLD, "reference_densify.npz"))
    pc = _model_from(fx, GaussianAdam)
    max_grad, min_opacity, extent, max_screen_size, pc.percent_dense = (float(x) for x in fx["args"])
    counts = densify.densify_and_prune(pc, max_grad, min_opacity, extent, max_screen_size, split_samples=torch.from_numpy(fx["samples"]))
    assert counts["points"] == fx["out_xyz"].shape[0] != fx["in_xyz"].shape[0] and type(pc.optimizer) is GaussianAdam
    _compare_model(pc, fx)
    for key, got in (("out_xyz_gradient_accum", pc.xyz_gradient_accum), ("out_denom", pc.denom), ("out_max_radii2D", pc.max_radii2D)):
        assert torch.equal(got.cpu(), torch.from_numpy(fx[key])), key
    _one_more_step(pc, 4)                                                 # the fused step runs on the new row count


def test_prune_only_replays_the_reference_method():
    fx = np.load(os.path.join(GOLD, "reference_prune_only.npz"))
    pc = _model_from(fx, GaussianAdam)
    min_opacity, size_thresh = (float(x) for x in fx["args"])
    _, _, mask, _ = densify.densify_masks(pc.xyz_gradient_accum, pc.denom, pc._scaling, pc._opacity, pc.max_radii2D, 0.0, 0.0, 1.0,
                                          min_opacity, size_thresh=size_thresh, raw_params=True)
    assert np.array_equal(mask.cpu().numpy(), fx["prune_mask"])                         # the mask, exact
    counts = densify.prune_only(pc, min_opacity, size_thresh)
    assert counts == {"pruned": int(fx["prune_mask"].sum()), "points": fx["out_xyz"].shape[0]}
    _compare_model(pc, fx, exact=True)                                                  # survivors are copies: the row order, exact
    for key, got in (("out_xyz_gradient_accum", pc.xyz_gradient_accum), ("out_denom", pc.denom), ("out_max_radii2D", pc.max_radii2D)):
        assert torch.equal(got.cpu(), torch.from_numpy(fx[key])), key
    _one_more_step(pc, 4)
    with pytest.raises(ValueError):
        densify.prune_only(pc, min_opacity, 0.0)
    # and on the reference's own optimizer class
    pc2 = _model_from(fx, torch.optim.Adam)
    densify.prune_only(pc2, min_opacity, size_thresh)
    _compare_model(pc2, fx, exact=True)


def test_two_identical_runs_are_bit_equal():
    vals, grads = _reference_groups(1000, 3, 51), _grad_sequence(1000, 3, 3, 52)
    a, oa = _run(GaussianAdam, vals, grads, dev())
    b, ob = _run(GaussianAdam, vals, grads, dev())
    for n in vals:
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), n
    for ga, gb in zip(oa.param_groups, ob.param_groups):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[ga["params"][0]][k], ob.state[gb["params"][0]][k])
