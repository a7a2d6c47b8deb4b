"""The step's guidance images and opacity losses as plain torch ops under autograd: the formulas of include/hgs_rast.h
(hgs_step_images_*), which are those of the reference's training step (threestudio/systems/GaussianDreamer.py:285-302,
:330-333, :359-366; threestudio/models/guidance/dual_branch_guidance.py:762-770).  Run in float64 it is the truth the
kernels are compared with, in float32 on the CPU the yardstick: a kernel's max |error| per tensor may be 4 x the float32
run's own, with a floor of 16 eps32 max|value| (the convention of tests/test_gpu_lbs.py).

It also carries the case table of tests/test_gpu_step_images.py, built from the kernels' chunk sizes."""
import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.finfo(np.float32).eps)
OUTPUTS = ("rgb", "depth", "loss_sparsity", "loss_opaque")
GRADS = {"all": OUTPUTS, "sparsity": ("loss_sparsity",), "rgb": ("rgb",)}


def formulas(render, depth, size):
    """render (B, 3, H, W), depth (B, 1, H, W) of one dtype -> dict of the seven results (differentiable)"""
    dmin = torch.amin(depth, dim=[1, 2, 3], keepdim=True)
    dmax = torch.amax(depth, dim=[1, 2, 3], keepdim=True)
    g = depth.max()
    nd = (depth - dmin) / (dmax - dmin + 1e-10)
    rgb = F.interpolate(render, size, mode="bilinear", align_corners=False)
    d3 = F.interpolate(nd.repeat(1, 3, 1, 1), size, mode="bilinear", align_corners=False)
    opacity = depth / (g + 1e-5)
    loss_sparsity = (opacity ** 2 + 0.01).sqrt().mean()
    x = opacity.clamp(1.0e-3, 1.0 - 1.0e-3)
    loss_opaque = F.binary_cross_entropy(x, x)
    return {"rgb": rgb, "depth": d3, "loss_sparsity": loss_sparsity, "loss_opaque": loss_opaque,
            "depth_min": dmin.reshape(-1), "depth_max": dmax.reshape(-1), "depth_global_max": g}


def run(render, depth, size, grads, dtype):
    """The formulas and their autograd in `dtype` on the CPU.  render, depth: float32 tensors (the inputs the kernels
    get); grads: {output name: incoming gradient} for the outputs the loss uses.  Returns float64 numpy arrays: the seven
    outputs, `grad_render` and `grad_depth` (None if no gradient reaches the input)."""
    r = render.detach().cpu().to(dtype).requires_grad_(True)
    d = depth.detach().cpu().to(dtype).requires_grad_(True)
    out = formulas(r, d, size)
    names = [n for n in OUTPUTS if n in grads]
    torch.autograd.backward([out[n] for n in names], [grads[n].detach().cpu().to(dtype) for n in names])
    res = {k: v.detach().double().numpy() for k, v in out.items()}
    res["grad_render"] = None if r.grad is None else r.grad.double().numpy()
    res["grad_depth"] = None if d.grad is None else d.grad.double().numpy()
    return res


# ---- inputs -------------------------------------------------------------------------------------------------------

CONTENTS = ("blob", "empty_view", "constant_view", "unique_min", "tie_max", "tie_global")


def _blob(B, H, W, g):
    """depth > 0 inside an ellipse of about 30 % of the area, 0 outside (a black background)"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = torch.zeros(B, 1, H, W)
    for b in range(B):
        cy, cx = (H - 1) * (0.4 + 0.2 * torch.rand(1, generator=g)), (W - 1) * (0.4 + 0.2 * torch.rand(1, generator=g))
        inside = ((yy - cy) / (0.31 * H + 0.5)) ** 2 + ((xx - cx) / (0.31 * W + 0.5)) ** 2 <= 1.0
        d[b, 0] = torch.where(inside, 1.0 + 1.5 * torch.rand(H, W, generator=g), torch.zeros(()))
    return d


def make_inputs(case):
    """-> (render, depth) float32 CPU tensors of the case"""
    B, H, W = case["B"], case["H"], case["W"]
    g = torch.Generator().manual_seed(case["seed"])
    render = torch.rand(B, 3, H, W, generator=g)
    kind = case["content"]
    depth = _blob(B, H, W, g)
    if kind == "empty_view":
        depth[B // 2] = 0.0
    elif kind == "constant_view":
        depth[B // 2] = 0.75
    elif kind == "unique_min":
        n = B * H * W
        depth = (0.5 + 2.0 * (torch.randperm(n, generator=g).float() + 0.25) / n).reshape(B, 1, H, W)
    elif kind == "tie_max":
        flat = depth[0].reshape(-1)
        flat[0] = flat[-1] = 2.75                     # above every blob value (< 2.5)
    elif kind == "tie_global":
        depth[0].reshape(-1)[H * W // 2] = 3.0
        depth[B - 1].reshape(-1)[H * W // 3] = 3.0
    return render, depth


def make_grads(case, dtype=torch.float32):
    """incoming gradients of the case, float32 values (rounded to `dtype` first, so that an fp16 run sees the same)"""
    B, h, w = case["B"], case["h"], case["w"]
    g = torch.Generator().manual_seed(case["seed"] + 1000)
    full = {"rgb": torch.randn(B, 3, h, w, generator=g).to(dtype).float(),
            "depth": torch.randn(B, 3, h, w, generator=g).to(dtype).float(),
            "loss_sparsity": torch.tensor(1.0),       # lambda_sparsity: 1. in configs/test.yaml
            "loss_opaque": torch.tensor(0.25)}
    return {k: full[k] for k in GRADS[case["grads"]]}


# ---- the case table -----------------------------------------------------------------------------------------------

# (H, W) -> (h, w), B: the shapes the resize can go wrong at
SIZES = (
    ((2, 2), (1, 1), 1),          # smallest
    ((4, 8), (2, 4), 2),          # 2:1
    ((6, 10), (3, 5), 3),         # 2:1 with a vector tail
    ((33, 47), (16, 23), 3),      # non-integer scale, odd sizes, i1 clamped at the edge
    ((32, 32), (32, 32), 2),      # identity
    ((64, 64), (4, 4), 1),        # 16:1
    ((37, 53), (1, 1), 2),        # collapse to one pixel
    ((256, 256), (128, 128), 8),  # many workgroups, many partials per view
)


def boundary_sizes(pixels_per_thread, pixels_per_workgroup, partials_per_view):
    """Shapes at N and N + 1 of each chunk size of the reductions: a view of exactly one thread's pixels and one more,
    one workgroup's chunk and one pixel more, as many chunks as a view has partials and one more (a workgroup then
    takes a second chunk), with full and with ragged last chunks."""
    t, c, p = pixels_per_thread, pixels_per_workgroup, partials_per_view
    out = {"thread": ((1, t), (1, t)), "thread+1": ((1, t + 1), (1, (t + 1) // 2 + 1)),
           "chunk": ((c // 32, 32), (c // 64, 16)), "chunk+1": ((1, c + 1), (1, c // 3))}
    rows = p * c // 256
    out["partials"] = ((rows, 256), (rows // 2, 128))                       # p chunks, all full
    out["partials+1"] = ((rows + c // 256, 256), ((rows + c // 256) // 2, 128))   # p + 1 chunks, 2:1
    out["partials+1-ragged"] = ((p * c // 255 + 1, 255), (rows // 3, 77))           # p + 1 chunks, the last one partial, H W % 4 != 0
    return out


def chunks_of(H, W, pixels_per_workgroup):
    return -(-H * W // pixels_per_workgroup)


def sweep_cases(pixels_per_thread, pixels_per_workgroup, partials_per_view):
    cases = []

    def add(tag, HW, hw, B, content="blob", grads="all"):
        cases.append({"id": f"{tag}-{HW[0]}x{HW[1]}to{hw[0]}x{hw[1]}-B{B}-{content}-{grads}", "tag": tag, "B": B, "H": HW[0],
                      "W": HW[1], "h": hw[0], "w": hw[1], "content": content, "grads": grads, "seed": 100 + len(cases)})
    for HW, hw, B in SIZES:
        add("size", HW, hw, B)
    for tag, (HW, hw) in boundary_sizes(pixels_per_thread, pixels_per_workgroup, partials_per_view).items():
        add(tag, HW, hw, 1 if HW[0] * HW[1] > 4096 else 2)
    for content in CONTENTS[1:]:
        add("content", (33, 47), (16, 23), 3, content)
        add("content", (6, 10), (3, 5), 2, content)
        add("content", (48, 40), (24, 20), 3, content)      # 2:1, W % 8 == 0: the 16-byte path, more than one chunk
    for grads in ("sparsity", "rgb"):
        for content in ("blob", "empty_view"):
            add("grads", (33, 47), (16, 23), 3, content, grads)
            add("grads", (48, 40), (24, 20), 2, content, grads)
    return cases
