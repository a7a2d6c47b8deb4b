"""View-parallel multi-GPU rendering: one process per GPU, views sharded round-robin,
Gaussian parameters replicated, ONE collective per step.

The reference renders its B views sequentially on one GPU and accumulates, per Gaussian,
  * parameter gradients (autograd sums them over views),
  * `radii` max over views                     (threestudio/systems/GaussianDreamer.py:253-256),
  * `viewspace_points.grad` summed over views   (GaussianDreamer.py:385-387),
so views are independent units.  Here rank r renders views r, r+G, ...;
each rank packs its per-Gaussian contribution into one (P, F) fp32 tensor
[means3D 3 | means2D 3 | sh 3M | opacity 1 | scales 3 | rotations 4 | radii 1]
and a single all-gather (RCCL over xGMI; gloo in the CPU tests) hands every rank all G
packs; the reduction (sum / max) is then done locally in rank order, so the result is
bit-identical on every rank and independent of arrival order.

A direct all-gather of a 6.8 MB pack rides the 7 point-to-point xGMI links in parallel
(about 45 us at 153 GB/s per link) - a ring all-reduce would be per-link bound.

With MORE than one view per rank the step is a pipeline (`render_views_parallel(..., pipeline=True)`,
the default then): round j = the views j*G .. j*G+G-1, one per rank; its packs are gathered by an
ASYNCHRONOUS collective (RCCL's own stream) while the ranks render round j+1, and the rounds are
chained by `reduce_gathered(gathered, acc_in=total)`:  total = ((total + rank 0) + rank 1) + ... -
exactly the left-to-right sum over the views in VIEW ORDER that the reference's serial loop forms
(GaussianDreamer.py:244-266, 385-391), bit for bit, on every rank.  Only the last round's
collective is exposed; with one view per rank there is nothing to hide it behind.

The rasterizer is passed in (`render_fn`) so the host logic is testable without a GPU;
the default is the HIP rasterizer and there is no CPU fallback in the product path.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import torch
import torch.distributed as dist

GRAD_KEYS = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")


def shard_views(num_views: int, rank: int, world: int) -> List[int]:
    """View v belongs to rank v mod world (frames of an animation shard the same way)."""
    return list(range(rank, num_views, world))


def pack_contribution(grads: Dict[str, torch.Tensor], radii: torch.Tensor) -> torch.Tensor:
    """(P, F) fp32 pack.  radii (int32) travel as exact fp32 integers (< 2^24)."""
    P = radii.shape[0]
    if radii.is_cuda and radii.dtype == torch.int32 and P > 0:
        from . import _lib          # one HIP pass instead of seven reshapes/casts and a cat
        return _lib.load_binding().pack_view_contribution(
            grads["means3D"], grads["means2D"], grads["shs"], grads["opacities"], grads["scales"],
            grads["rotations"], radii)
    cols = [grads[k].reshape(P, -1).float() for k in GRAD_KEYS]
    cols.append(radii.reshape(P, 1).float())
    return torch.cat(cols, dim=1).contiguous()


def reduce_gathered_unpacked(gathered: torch.Tensor, acc_in: Optional[torch.Tensor], shapes: Dict[str, torch.Size]):
    """The LAST reduction of a step with the unpack fused in (one HIP pass: include/hgs_rast.h
    hgs_reduce_view_packs_unpack): (world, P, F) [+ running total] -> (grads dict, radii int32) - the same bits as
    `unpack_contribution(reduce_gathered(gathered, acc_in), shapes)`, without the (P, F) intermediate and the slicing /
    rounding kernels behind it."""
    if gathered.is_cuda and gathered.dim() == 3:
        from . import _lib
        m3, m2, sh, op, sc, ro, radii = _lib.load_binding().reduce_view_packs_unpack(gathered, acc_in)
        out = {"means3D": m3, "means2D": m2, "shs": sh, "opacities": op, "scales": sc, "rotations": ro}
        return {k: out[k].reshape(shapes[k]) for k in GRAD_KEYS}, radii
    return unpack_contribution(reduce_gathered(gathered, acc_in), shapes)


def unpack_contribution(pack: torch.Tensor, shapes: Dict[str, torch.Size]):
    out, c = {}, 0
    P = pack.shape[0]
    for k in GRAD_KEYS:
        n = int(torch.Size(shapes[k]).numel() // max(P, 1)) if P else 0
        out[k] = pack[:, c:c + n].reshape(shapes[k])
        c += n
    radii = pack[:, c].round().to(torch.int32)
    return out, radii


def _host_staged(t: torch.Tensor, group=None) -> bool:
    """gloo moves host memory: device tensors are staged through the host for it (the debugging /
    single-GPU test configuration: two ranks on ONE device cannot form an RCCL communicator)."""
    return t.is_cuda and dist.get_backend(group) == "gloo"


class _Gather:
    """An all-gather of one rank's (P, F) pack that may still be in flight."""

    def __init__(self, pack: torch.Tensor, group=None, async_op: bool = False):
        world = dist.get_world_size(group)
        self.shape = (world,) + tuple(pack.shape)
        self.device = pack.device
        self.staged = _host_staged(pack, group)
        src = pack.cpu() if self.staged else pack
        # flat (world*P, F) output: the concatenation form is accepted by both RCCL and gloo
        self.flat = torch.empty((world * pack.shape[0],) + tuple(pack.shape[1:]), dtype=pack.dtype, device=src.device)
        self.src = src                                # (kept alive until the collective has read it)
        self.work = dist.all_gather_into_tensor(self.flat, src, group=group, async_op=async_op)

    def result(self) -> torch.Tensor:
        if self.work is not None:
            self.work.wait()                          # RCCL: the CURRENT stream waits for the collective's stream
            self.work = None
        flat = self.flat.to(self.device) if self.staged else self.flat
        return flat.view(self.shape)


PackGather = _Gather        # public name: `PackGather(pack, async_op=True)` ... `.result()` (bench.py, pipelines)


def allgather(pack: torch.Tensor, group=None) -> torch.Tensor:
    """THE collective of a step: every rank's (P, F) pack -> (world, P, F) on every rank."""
    return _Gather(pack, group).result()


def reduce_gathered(gathered: torch.Tensor, acc_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Local reduction in rank order (bit-identical on every rank): gradient columns are summed,
    the last column (radii) takes the max.  `acc_in` (P, F): the running total of the step's earlier
    collectives - the chain then continues ((acc_in + rank 0) + rank 1) + ..."""
    world = gathered.shape[0]
    if gathered.is_cuda and gathered.dim() == 3:
        # one HIP pass (rank-order sum, max on the radii column) instead of 2 (world - 1) strided
        # torch kernels launched from a Python loop
        from . import _lib
        return _lib.load_binding().reduce_view_packs(gathered, acc_in)
    if acc_in is None:
        total, first = gathered[0].clone(), 1
    else:
        total, first = acc_in.clone(), 0
    for r in range(first, world):                 # fixed order => deterministic sum
        total[:, :-1] += gathered[r][:, :-1]
        total[:, -1] = torch.maximum(total[:, -1], gathered[r][:, -1])
    return total


def scatter_reduce_gather(pack: torch.Tensor, group=None) -> torch.Tensor:
    """Same result as `reduce_gathered(allgather(pack))` - bit for bit, rank-ordered - with an eighth of
    the traffic at world 8: the rows are cut into `world` shards; an all-to-all hands rank r every
    rank's copy of shard r (P/world rows from each peer: one message per point-to-point xGMI link),
    rank r reduces its shard locally in rank order (the same HIP pass), and ONE all-gather of the
    reduced shards completes the tensor on every rank.  Per rank 2 (world-1)/world packs cross the
    links instead of (world-1) packs; at world 8 and P = 100k that is 12 MB instead of 48 MB."""
    world = dist.get_world_size(group)
    P, F = pack.shape
    Ps = (P + world - 1) // world
    if Ps * world != P:                                     # pad to a multiple of the world size
        padded = pack.new_zeros((Ps * world, F))
        padded[:P] = pack
        pack = padded
    dev, staged = pack.device, _host_staged(pack, group)
    src = pack.contiguous().cpu() if staged else pack.contiguous()
    recv = torch.empty((world, Ps, F), dtype=pack.dtype, device=src.device)
    dist.all_to_all_single(recv.view(world * Ps, F), src, group=group)
    shard = reduce_gathered(recv.to(dev) if staged else recv)      # (Ps, F): rank-ordered sum / max of MY rows
    shard = shard.contiguous().cpu() if staged else shard.contiguous()
    full = torch.empty((world * Ps, F), dtype=pack.dtype, device=shard.device)
    dist.all_gather_into_tensor(full, shard, group=group)
    return (full.to(dev) if staged else full)[:P]


COLLECTIVE_MODES = ("allgather", "scatter")


def default_collective(world: int) -> str:
    """What "auto" means where nobody has timed the two modes on the node at hand: the single all-gather up to four ranks,
    `scatter` from eight ranks on - per rank (world - 1) packs cross the point-to-point xGMI links in an all-gather, 2
    (world - 1) / world in the scatter form (7 vs 1.75 packs at world 8), for one more collective's latency.
    (bench.py --collective auto times both and takes the faster one.)"""
    return "scatter" if world >= 8 else "allgather"


def allgather_reduce_unpacked(pack: torch.Tensor, shapes: Dict[str, torch.Size], group=None, mode: str = "allgather"):
    """`allgather_reduce` + `unpack_contribution` with the last reduction and the unpack as ONE pass where the mode ends
    in a local reduction of gathered packs (mode "allgather"; "scatter" ends in an all-gather of reduced shards: its
    result is unpacked as before)."""
    if mode == "allgather" and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        return reduce_gathered_unpacked(allgather(pack, group), None, shapes)
    return unpack_contribution(allgather_reduce(pack, group, mode), shapes)


def allgather_reduce(pack: torch.Tensor, group=None, mode: str = "allgather") -> torch.Tensor:
    """The collective of a step: every rank's pack in, the rank-ordered reduction out (identical bits
    on every rank).  mode "allgather": ONE all-gather of the packs + local reduction;
    mode "scatter": all-to-all of shards + local reduction + one all-gather of the reduced shards
    (`scatter_reduce_gather`) - fewer bytes per link, one more collective."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return pack
    if mode == "scatter":
        return scatter_reduce_gather(pack, group)
    if mode != "allgather":
        raise ValueError(f"unknown collective mode {mode!r}")
    return reduce_gathered(allgather(pack, group))


def render_views_parallel(cameras: Sequence, params: Dict[str, torch.Tensor], bg: torch.Tensor,
                          sh_degree: int, loss_grad_fn: Callable, render_fn: Optional[Callable] = None,
                          group=None, gather_images: bool = False, collective: str = "allgather",
                          pipeline: Optional[bool] = None, batched: bool = False,
                          render_batch_fn: Optional[Callable] = None):
    """One training-style step over `cameras` (the global list, identical on every rank).

    params        replicated leaf tensors: means3D, shs, opacities, scales, rotations
    loss_grad_fn  (view_index, color, depth, alpha) -> (dL/dcolor, dL/ddepth, dL/dalpha)
    render_fn     (camera, params, means2D, bg, sh_degree) -> (color, radii, depth, alpha);
                  defaults to the HIP rasterizer.
    pipeline      True: one asynchronous all-gather per ROUND of views (one view per rank), overlapped with
                  the render of the next round, rounds chained in view order (module docstring) - the BITS of the
                  reference's serial loop;
                  False: the rank's views are summed locally and ONE collective ends the step
                  (`collective` = "allgather" | "scatter"); None: pipeline iff a rank renders > 1 view (and the
                  collective is the default all-gather).
    batched       True (excludes pipeline): the rank's views go through ONE batched rasterize call
                  (`rasterize_gaussians_batch`: one launch set, 124 instead of 171 us per view at configs[1]; the kernel
                  sums the rank's parameter gradients in view order) and ONE collective ends the step.  Deterministic and
                  identical on every rank, but the sum is associated per rank first - (v0 + vG + ..) + (v1 + ..) + .. -
                  so it agrees with the serial loop to rounding, not bit for bit; `pipeline=True` keeps the bits.
    render_batch_fn  (cameras, params, means2D (B,P,3), bg, sh_degree) -> (color (B,..), radii (B,P), depth, alpha);
                  defaults to the batched HIP call.
    Returns (grads dict summed over ALL views, radii max over all views, local outputs).
    """
    if render_fn is None:
        render_fn = hip_render_fn
    rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    mine = shard_views(len(cameras), rank, world)
    rounds = (len(cameras) + world - 1) // world
    if collective == "auto":
        collective = default_collective(world) if not pipeline else "allgather"
    if batched and pipeline:
        raise ValueError("batched=True renders the rank's views in one call: there are no rounds to pipeline")
    if pipeline is None:                                    # (an explicit collective mode is honoured: it needs the one-collective form)
        pipeline = rounds > 1 and not batched and collective == "allgather"
    if pipeline and collective != "allgather":
        raise ValueError(f"pipeline=True gathers one pack per round with all_gather; collective={collective!r} applies to "
                         f"pipeline=False only")
    leaves = {k: params[k].detach().requires_grad_(True) for k in
              ("means3D", "shs", "opacities", "scales", "rotations")}
    P = leaves["means3D"].shape[0]
    dev = leaves["means3D"].device
    names = ("means3D", "shs", "opacities", "scales", "rotations", "means2D")
    shapes = {k: leaves[k].shape for k in leaves}
    shapes["means2D"] = leaves["means3D"].shape
    outputs = []

    # On the HIP path the rasterizer's last backward kernel writes the pack itself (rasterizer.packed_gradients): no
    # pack kernel, no second pass over the six gradient tensors on the exposed path of a step.  That pack holds the
    # gradients w.r.t. the RASTERIZER's inputs, which are the leaves only when the default functions hand the leaves
    # straight to one rasterizer call; a custom render_fn (activations, re-posed means, a subset, two calls) packs
    # its autograd result instead.
    if batched:
        hip_pack = dev.type == "cuda" and render_batch_fn in (None, hip_render_batch_fn)
    else:
        hip_pack = dev.type == "cuda" and render_fn is hip_render_fn
    if hip_pack:
        from .rasterizer import packed_gradients
    F = 15 + 3 * int(leaves["shs"].shape[1]) if leaves["shs"].dim() == 3 else -1

    def grads_of(outs, tens, gouts):
        """-> (gradient tuple, pack or None)"""
        if not hip_pack or not outs:
            return torch.autograd.grad(outs, tens, gouts, allow_unused=True), None
        with packed_gradients() as pg:
            gl = torch.autograd.grad(outs, tens, gouts, allow_unused=True)
            pack = pg.take()
        # (a pack that does not fit the leaves - another call's, or none at all - is not used: the caller packs `gl`)
        if pack is not None and (tuple(pack.shape) != (P, F) or pack.dtype != torch.float32 or not pack.is_contiguous()
                                 or pack.device != dev):
            pack = None
        return gl, pack

    def one_view(v, want_pack=False):
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
        color, radii, depth, alpha = render_fn(cameras[v], leaves, means2D, bg, sh_degree)
        gc, gd, ga = loss_grad_fn(v, color.detach(), depth.detach(), alpha.detach())
        tens = [leaves[k] for k in names[:-1]] + [means2D]
        outs, gouts = [], []
        for o, g in ((color, gc), (depth, gd), (alpha, ga)):
            if g is not None:
                outs.append(o); gouts.append(g)
        gl, pack = grads_of(outs, tens, gouts)
        outputs.append((v, color.detach(), depth.detach(), alpha.detach()))
        g = {k: (g if g is not None else torch.zeros(shapes[k], dtype=leaves["means3D"].dtype, device=dev))
             for k, g in zip(names, gl)}
        if want_pack:
            return pack if pack is not None else pack_contribution(g, radii)
        return g, radii

    if batched:
        acc = {k: torch.zeros(shapes[k], dtype=leaves["means3D"].dtype, device=dev) for k in names}
        radii_max = torch.zeros(P, dtype=torch.int32, device=dev)
        if mine:
            fn = render_batch_fn if render_batch_fn is not None else hip_render_batch_fn
            means2D = torch.zeros((len(mine),) + tuple(leaves["means3D"].shape), dtype=leaves["means3D"].dtype, device=dev,
                                  requires_grad=True)
            color, radii, depth, alpha = fn([cameras[v] for v in mine], leaves, means2D, bg, sh_degree)
            outs, gouts = [], []
            per_view = [loss_grad_fn(v, color[i].detach(), depth[i].detach(), alpha[i].detach()) for i, v in enumerate(mine)]
            for o, col in ((color, 0), (depth, 1), (alpha, 2)):
                if any(pv[col] is not None for pv in per_view):
                    outs.append(o)
                    gouts.append(torch.stack([pv[col] if pv[col] is not None else torch.zeros_like(o[i])
                                              for i, pv in enumerate(per_view)]))
            tens = [leaves[k] for k in names[:-1]] + [means2D]
            gl, bpack = grads_of(outs, tens, gouts)
            for i, v in enumerate(mine):
                outputs.append((v, color[i].detach(), depth[i].detach(), alpha[i].detach()))
            if bpack is None:
                for k, g in zip(names, gl):
                    if g is not None:
                        acc[k] = g if k != "means2D" else g.sum(0)       # (screen-space gradients: summed over the rank's views)
                radii_max = radii.max(dim=0).values.to(torch.int32)
        else:
            bpack = None
        if bpack is None:
            bpack = pack_contribution(acc, radii_max)
        grads, radii_all = allgather_reduce_unpacked(bpack, {k: shapes[k] for k in GRAD_KEYS}, group, mode=collective)
        if gather_images and world > 1:
            outputs = gather_view_images(outputs, len(cameras), group)
        return grads, radii_all, outputs
    elif not pipeline:
        if len(mine) == 1:                    # one view per rank (north_star's configs[2]): the pack comes from the backward itself
            pack = one_view(mine[0], want_pack=True)
        else:
            acc = {k: torch.zeros(shapes[k], dtype=leaves["means3D"].dtype, device=dev) for k in names}
            radii_max = torch.zeros(P, dtype=torch.int32, device=dev)
            for v in mine:
                g, radii = one_view(v)
                for k in names:
                    acc[k] += g[k]
                radii_max = torch.maximum(radii_max, radii)
            pack = pack_contribution(acc, radii_max)
        grads, radii_all = allgather_reduce_unpacked(pack, {k: shapes[k] for k in GRAD_KEYS}, group, mode=collective)
        if gather_images and world > 1:
            outputs = gather_view_images(outputs, len(cameras), group)
        return grads, radii_all, outputs
    else:
        # round j: every rank contributes the pack of its view j * world + rank (zeros beyond the last view:
        # x + 0 = x exactly), gathered while round j + 1 is rendered; chained in view order
        total, pending = None, None
        zero_pack = None
        for j in range(rounds):
            v = j * world + rank
            if v < len(cameras):
                pack = one_view(v, want_pack=True)
            else:
                if zero_pack is None:
                    F = sum(int(torch.Size(shapes[k]).numel() // max(P, 1)) for k in GRAD_KEYS) + 1
                    zero_pack = torch.zeros((P, F), dtype=torch.float32, device=dev)
                pack = zero_pack
            if world > 1:
                started = _Gather(pack, group, async_op=True)
                if pending is not None:                     # round j - 1 has had a whole render to arrive
                    total = reduce_gathered(pending.result(), total)
                pending = started
            else:
                total = pack.clone() if total is None else reduce_gathered(pack[None], total)
        if pending is not None:                             # the last round's reduction writes the gradient tensors itself
            grads, radii_all = reduce_gathered_unpacked(pending.result(), total, {k: shapes[k] for k in GRAD_KEYS})
            if gather_images and world > 1:
                outputs = gather_view_images(outputs, len(cameras), group)
            return grads, radii_all, outputs
        if total is None:                                   # no view at all: the zero contribution
            F = sum(int(torch.Size(shapes[k]).numel() // max(P, 1)) for k in GRAD_KEYS) + 1
            total = torch.zeros((P, F), dtype=torch.float32, device=dev)
    grads, radii_all = unpack_contribution(total, {k: shapes[k] for k in GRAD_KEYS})
    if gather_images and world > 1:
        outputs = gather_view_images(outputs, len(cameras), group)
    return grads, radii_all, outputs


def gather_view_images(outputs, num_views: int, group=None):
    """Optional forward collective: all-gather the [color|depth|alpha] slab (5,H,W) of each
    rank's views so every rank holds all views (only needed when the consumer is not
    view-separable; the SDS loss is)."""
    world = dist.get_world_size(group)
    per_rank = (num_views + world - 1) // world
    if num_views < world:
        # the SAME test on every rank, before the collective: a rank without a view cannot size its slab, and raising
        # only there would leave the other ranks inside the all-gather
        raise ValueError(f"gather_view_images: {num_views} views for {world} ranks - every rank needs at least one view")
    v0, c0, d0, a0 = outputs[0]
    slab = torch.zeros((per_rank, 5) + tuple(c0.shape[1:]), dtype=c0.dtype, device=c0.device)
    for i, (_, c, d, a) in enumerate(outputs):
        slab[i, :3], slab[i, 3:4], slab[i, 4:5] = c, d, a
    staged = _host_staged(slab, group)
    src = slab.cpu() if staged else slab
    flat = torch.empty((world * slab.shape[0],) + tuple(slab.shape[1:]), dtype=slab.dtype, device=src.device)
    dist.all_gather_into_tensor(flat, src, group=group)
    if staged:
        flat = flat.to(slab.device)
    allslab = flat.view((world,) + tuple(slab.shape))
    res = []
    for v in range(num_views):
        s = allslab[v % world, v // world]
        res.append((v, s[:3], s[3:4], s[4:5]))
    return res


def hip_render_batch_fn(cams, leaves, means2D, bg, sh_degree):
    """Default render_batch_fn: the views of one rank in ONE batched HIP call (hgs_forward_batch / hgs_backward_batch)."""
    import math
    from .rasterizer import GaussianRasterizationSettings, rasterize_gaussians_batch
    rsl = [GaussianRasterizationSettings(
        int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0,
        cam.world_view_transform, cam.full_proj_transform, sh_degree, cam.camera_center, False, False) for cam in cams]
    return rasterize_gaussians_batch(leaves["means3D"], means2D, leaves["shs"], None, leaves["opacities"], leaves["scales"],
                                     leaves["rotations"], None, rsl)


def hip_render_fn(cam, leaves, means2D, bg, sh_degree):
    """Default render_fn: the HIP rasterizer behind the reference API."""
    import math
    from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(
        int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5),
        math.tan(cam.FoVy * 0.5), bg, 1.0, cam.world_view_transform, cam.full_proj_transform,
        sh_degree, cam.camera_center, False, False)
    return GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=means2D, shs=leaves["shs"],
                                  opacities=leaves["opacities"], scales=leaves["scales"],
                                  rotations=leaves["rotations"])
