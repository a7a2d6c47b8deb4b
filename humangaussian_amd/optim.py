"""The optimizer step of the training loop as ONE HIP launch (csrc/optim.hip, `hgs_adam_step`).

The reference builds `torch.optim.Adam(l, lr=0.0, eps=1e-15)` over six parameter groups of one tensor each
(gaussiansplatting/scene/gaussian_model.py:156-165).  Torch's multi-tensor path batches per group, so one tensor per
group means one chain of elementwise kernels per group and step.  `GaussianAdam` is that optimizer - same constructor,
same `param_groups`, same per-parameter state - whose `step` hands every eligible parameter of every group to one kernel
launch.  The one line a caller adds after `training_setup`:

    pc.optimizer = GaussianAdam.from_optimizer(pc.optimizer)
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch.optim import adam as _torch_adam

from . import _lib

_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable")


class GaussianAdam(torch.optim.Adam):
    """`torch.optim.Adam` with the step of all groups fused into one HIP launch.

    State per parameter is what the installed torch's non-fused, non-capturable Adam creates: `step` (a float32 scalar
    tensor on the CPU), `exp_avg`, `exp_avg_sq`.  So `state_dict` / `load_state_dict`, the reference's optimizer surgery
    (`replace_tensor_to_optimizer`, `_prune_optimizer`, `cat_tensors_to_optimizer`), `densify.densify_and_prune` and
    torch's own `Adam.step` all work on it and can continue from it.

    Which parameters take the HIP path: fp32, contiguous, on a HIP device, with a dense fp32 contiguous gradient and
    moments of the same kind, in a group whose `lr` / `betas` are Python numbers.  `lr`, `betas` and `eps` are read from
    the group at every call (learning-rate schedules keep working).  Parameters with `grad is None` are skipped as torch
    skips them.  Every other parameter takes torch's own single-tensor Adam for that parameter; on a machine without a
    GPU the class is therefore exactly `torch.optim.Adam`.

    Refused at construction (ValueError): `amsgrad`, `maximize`, `capturable`, `differentiable`, `fused=True`, a non-zero
    `weight_decay` - none of which the reference uses.  `_step_supports_amp_scaling` is not set: a `GradScaler` treats
    the class like plain Adam (unscale first, skip the step on inf).

    `step(visibility=mask)`: `mask` is a bool or uint8 tensor with one entry per Gaussian (row); rows whose entry is zero
    are left untouched - parameter and both moments keep their bits - while the step count and with it the bias
    correction stay global.  This differs from the sparse Adam of upstream 3DGS's accelerated rasterizer, which skips
    the same rows but applies no bias correction at all: here a row that is visible in every step gets exactly the
    dense result.  Dense (no mask) is the default because it is what the reference runs: its Adam decays the moments of
    every Gaussian every step, seen or not.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         foreach=foreach, maximize=maximize, capturable=capturable, differentiable=differentiable,
                         fused=fused, decoupled_weight_decay=decoupled_weight_decay)

    def add_param_group(self, param_group):
        # (the constructor adds every group through here, with the defaults filled in)
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        bad = [k for k in _REFUSED if group.get(k)]
        if group.get("fused"):
            bad.append("fused")
        if group.get("weight_decay", 0) != 0:
            bad.append("weight_decay")
        if bad:
            self.param_groups.pop()
            raise ValueError(f"GaussianAdam does not support {', '.join(bad)}: use torch.optim.Adam")

    @classmethod
    def from_optimizer(cls, adam: torch.optim.Adam) -> "GaussianAdam":
        """Adopts the groups (every key, `name` included) and the LIVE state of an existing `torch.optim.Adam`: the same
        parameter objects and the same moment tensors, no copy.  The old optimizer object should be dropped."""
        if not isinstance(adam, torch.optim.Adam):
            raise TypeError("GaussianAdam.from_optimizer expects a torch.optim.Adam")
        d = adam.defaults
        new = cls([dict(g, params=list(g["params"])) for g in adam.param_groups], lr=d["lr"], betas=d["betas"],
                  eps=d["eps"], weight_decay=d["weight_decay"], amsgrad=d["amsgrad"], foreach=d.get("foreach"),
                  maximize=d["maximize"], capturable=d["capturable"], differentiable=d["differentiable"],
                  fused=d.get("fused"), decoupled_weight_decay=d.get("decoupled_weight_decay", False))
        for p, st in adam.state.items():
            new.state[p] = st
        return new

    @staticmethod
    def _hip_ok(p: torch.Tensor, state: dict, group: dict) -> bool:
        g = p.grad

        def plain(t):
            return t.layout == torch.strided and t.dtype == torch.float32 and t.is_contiguous() and t.device == p.device

        return (p.device.type == "cuda" and torch.version.hip is not None and plain(p) and plain(g)
                and plain(state["exp_avg"]) and plain(state["exp_avg_sq"])
                and state["exp_avg"].shape == p.shape and state["exp_avg_sq"].shape == p.shape and g.shape == p.shape
                and state["step"].device.type == "cpu"
                and not torch.is_tensor(group["lr"]) and not any(torch.is_tensor(b) for b in group["betas"]))

    @torch.no_grad()
    def step(self, closure=None, visibility: Optional[torch.Tensor] = None):
        """One Adam step.  `visibility`: see the class docstring."""
        self._cuda_graph_capture_health_check()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if visibility is not None:          # refused before any state changes
            if not torch.is_tensor(visibility) or visibility.dtype not in (torch.bool, torch.uint8):
                raise ValueError("visibility must be a bool or uint8 tensor")
            for group in self.param_groups:
                for p in group["params"]:
                    if p.grad is not None and (p.dim() < 1 or p.shape[0] != visibility.numel()):
                        raise ValueError(f"visibility has {visibility.numel()} entries, a parameter has shape {tuple(p.shape)}")
        by_device = {}          # device -> (params, grads, exp_avgs, exp_avg_sqs, scalars)
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            rest = ([], [], [], [], [])
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:          # what torch's Adam._init_group creates without `capturable` / `fused`
                    state["step"] = torch.tensor(0.0, dtype=_torch_adam._get_scalar_dtype())
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if not self._hip_ok(p, state, group):
                    for lst, x in zip(rest, (p, p.grad, state["exp_avg"], state["exp_avg_sq"], state["step"])):
                        lst.append(x)
                    continue
                state["step"] += 1
                t = state["step"].item()                                  # (a CPU scalar: no device round trip)
                scalars = (group["lr"] / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t), 1.0 - beta1, beta2,
                           1.0 - beta2, group["eps"])
                lists = by_device.setdefault(p.device, ([], [], [], [], []))
                for lst, x in zip(lists, (p, p.grad, state["exp_avg"], state["exp_avg_sq"], scalars)):
                    lst.append(x)
            if rest[0]:
                if visibility is not None:
                    raise ValueError("visibility needs every parameter on the HIP path (fp32, contiguous, on the GPU)")
                _torch_adam.adam(rest[0], rest[1], rest[2], rest[3], [], rest[4], foreach=False, capturable=False,
                                 differentiable=False, fused=False, grad_scale=None, found_inf=None,
                                 has_complex=any(torch.is_complex(q) for q in rest[0]),
                                 decoupled_weight_decay=group.get("decoupled_weight_decay", False), amsgrad=False,
                                 beta1=beta1, beta2=beta2, lr=group["lr"], weight_decay=0, eps=group["eps"],
                                 maximize=False)
        for dev, (params, grads, exp_avgs, exp_avg_sqs, scalars) in by_device.items():
            vis = None
            if visibility is not None:
                vis = visibility.to(dev).reshape(-1).contiguous()
            _lib.load_binding().adam_step(params, grads, exp_avgs, exp_avg_sqs, scalars, vis)
        return loss
