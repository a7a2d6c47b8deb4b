"""Generates tests/golden/reference_prune_only.npz: the reference's OWN `GaussianModel.prune_only`
(gaussiansplatting/scene/gaussian_model.py:426-432, with the `prune_points` and `_prune_optimizer` it calls) run on a
small model with a live Adam state and non-trivial densification statistics: every input (raw parameters, both Adam
moments, the statistics, the arguments), the mask `prune_points` received and every output.  Made the way
make_densify_fixture.py makes its file (same model construction, the reference's `device="cuda"` factory calls redirected
to the CPU), arrays only.  Run where the reference tree exists:

    python tests/golden/make_prune_only_fixture.py            # (re)write the fixture
    python tests/golden/make_prune_only_fixture.py --check    # re-run the reference method, compare with the committed file

tests/test_gpu_optim.py replays the state through humangaussian_amd.densify.prune_only on the GPU (mask / row order
exact, tensors <= 1e-6); tests/test_optim_cpu.py checks the file against the method's definition in plain indexing."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_densify_fixture import GROUPS, REF, ROOT, _import_model  # noqa: E402

ARGS = dict(min_opacity=0.05, size_thresh=0.05)
PATH = os.path.join(ROOT, "tests", "golden", "reference_prune_only.npz")


def available() -> bool:
    return os.path.isdir(os.path.join(REF, "gaussiansplatting"))


def run():
    """-> dict of numpy arrays (inputs `in_*`, outputs `out_*`, `prune_mask`, `args`)."""
    GaussianModel = _import_model()
    saved = torch.zeros
    torch.zeros = lambda *a, **k: saved(*a, **{kk: ("cpu" if kk == "device" else vv) for kk, vv in k.items()})
    try:
        P, deg = 600, 1
        g = torch.Generator().manual_seed(91)
        pc = GaussianModel(deg)
        pc._xyz = torch.nn.Parameter((torch.rand(P, 3, generator=g) - 0.5) * 1.2)
        pc._features_dc = torch.nn.Parameter(torch.randn(P, 1, 3, generator=g) * 0.8)
        pc._features_rest = torch.nn.Parameter(torch.randn(P, (deg + 1) ** 2 - 1, 3, generator=g) * 0.3)
        pc._scaling = torch.nn.Parameter(torch.log(0.02 * torch.exp(1.2 * torch.randn(P, 3, generator=g))))
        pc._rotation = torch.nn.Parameter(torch.randn(P, 4, generator=g))
        pc._opacity = torch.nn.Parameter(torch.logit(0.01 + 0.98 * torch.rand(P, 1, generator=g)))
        pc.spatial_lr_scale = 1.0
        targs = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6,
                                      position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025,
                                      opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
        pc.training_setup(targs)
        for _ in range(3):                                       # a live Adam state: three steps on random gradients
            for _, attr in GROUPS:
                p = getattr(pc, attr)
                p.grad = torch.randn(p.shape, generator=g) * 0.1
            pc.optimizer.step()
        pc.xyz_gradient_accum = torch.rand(P, 1, generator=g) * 0.3
        pc.denom = torch.randint(0, 8, (P, 1), generator=g).float()
        pc.max_radii2D = torch.rand(P, generator=g) * 40.0
        out = {}
        for name, attr in GROUPS:
            p = getattr(pc, attr)
            st = pc.optimizer.state[p]
            out["in" + attr] = p.detach().numpy().copy()
            out["in_exp_avg_" + name] = st["exp_avg"].numpy().copy()
            out["in_exp_avg_sq_" + name] = st["exp_avg_sq"].numpy().copy()
        out["in_xyz_gradient_accum"], out["in_denom"] = pc.xyz_gradient_accum.numpy().copy(), pc.denom.numpy().copy()
        out["in_max_radii2D"] = pc.max_radii2D.numpy().copy()
        masks = []
        prune_points = pc.prune_points

        def recording(mask):
            masks.append(mask.detach().clone())
            return prune_points(mask)
        pc.prune_points = recording
        pc.prune_only(ARGS["min_opacity"], ARGS["size_thresh"])
        assert len(masks) == 1
        out["prune_mask"] = masks[0].numpy().copy()
        for name, attr in GROUPS:
            p = getattr(pc, attr)
            group = next(gr for gr in pc.optimizer.param_groups if gr["name"] == name)
            assert group["params"][0] is p
            st = pc.optimizer.state[p]
            out["out" + attr] = p.detach().numpy().copy()
            out["out_exp_avg_" + name] = st["exp_avg"].numpy().copy()
            out["out_exp_avg_sq_" + name] = st["exp_avg_sq"].numpy().copy()
        out["out_xyz_gradient_accum"], out["out_denom"] = pc.xyz_gradient_accum.numpy().copy(), pc.denom.numpy().copy()
        out["out_max_radii2D"] = pc.max_radii2D.numpy().copy()
        out["args"] = np.array([ARGS["min_opacity"], ARGS["size_thresh"]], np.float64)
        return out
    finally:
        torch.zeros = saved


def check(res=None):
    """The committed file is what the reference method produces (bit for bit)."""
    res = run() if res is None else res
    fx = np.load(PATH)
    assert sorted(fx.files) == sorted(res)
    for k in fx.files:
        assert np.array_equal(fx[k], res[k]), k
    n_in, n_out = res["in_xyz"].shape[0], res["out_xyz"].shape[0]
    assert 0 < n_out < n_in and int(res["prune_mask"].sum()) == n_in - n_out


if __name__ == "__main__":
    if "--check" in sys.argv:
        check()
        print("the committed", PATH, "is what the reference method produces")
        sys.exit(0)
    res = run()
    np.savez_compressed(PATH, **res)
    print("wrote", PATH, "points", res["in_xyz"].shape[0], "->", res["out_xyz"].shape[0])
