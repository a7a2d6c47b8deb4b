"""Device time of `GaussianField.sample` (hgs_fsample: density, normal and colour of the density field at arbitrary points)
at the vertices of the avatar's own mesh: 100 000 Gaussians on the body cloud, resolution 128, 16 blocks per axis.

  sample          field.sample(vertices, colors, normalized=True): binning (3 launches) + evaluation
  field_eval      hgs_field_eval on the same plan (list order + fill + the 128^3 evaluation): the yardstick - the same inner
                  loop with one accumulator, shared by two samples, where the point kernel has seven for one point
  torch_blocks    the same sums in torch ops, block by block: gather the block's list, evaluate the block's points densely

Not part of bench.py.  Per measurement WINDOWS windows of warm calls, device events around a window / reps = microseconds
per call; the median over the windows with their min and max.  `pairs` = (point, listed Gaussian) pairs a call evaluates:
for the samples the sum over the points of their block's list length, for the field 2 x the (thread, record) steps it
takes, i.e. split^3 x the sum of the list lengths.  Nothing here is a gate.

    python tools/field_sample_bench.py [--out profiles/field_sample.json] [--commit ID]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P, RES, NB, RELAX = 100_000, 128, 16, 1.5
WARMUP, WINDOWS, REPS, REPS_TORCH = 10, 5, 50, 2


def avatar(n, seed):
    """The cloud of the field's own timing record (tests/test_gpu_fields.py): the humanoid of synth, anisotropic scales"""
    from humangaussian_amd import synth
    rng = np.random.default_rng(seed)
    xyz = synth.humanoid_points(n, seed=seed).astype(np.float32)
    scaling = (0.012 * np.exp(0.5 * rng.normal(size=(n, 3)))).astype(np.float32)
    rotation = rng.normal(size=(n, 4)).astype(np.float32)
    opacity = (0.002 + 0.95 * rng.uniform(size=(n, 1))).astype(np.float32)
    return xyz, opacity, scaling, rotation


def windows(run, reps, warmup=WARMUP):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return out


def entry(us, reps, pairs=None):
    med = statistics.median(us)
    e = {"device_us_per_call": med, "device_us_per_call_min_max": [min(us), max(us)], "reps": reps, "windows": WINDOWS}
    if pairs is not None:
        e["pairs"] = int(pairs)
        e["pairs_per_s"] = pairs / (med * 1e-6)
    return e


def torch_blocks(cloud, center, scale, pts, colors):
    """density, G and colour sums of `pts` (normalised) in torch ops: per block that holds points, its list gathered and its
    points evaluated densely (written from the definition in include/hgs_rast.h)."""
    xyz, opacity, scaling, rotation = cloud
    keep = (opacity.reshape(-1) > 0.005) & torch.isfinite(xyz).all(1)
    x, s, q, o, c = (xyz[keep] - center) * scale, scaling[keep] * scale, rotation[keep], opacity.reshape(-1)[keep], colors[keep]
    q = q / q.norm(dim=1, keepdim=True)
    r, i, j, k = q.unbind(1)
    R = torch.stack([1 - 2 * (j * j + k * k), 2 * (i * j - r * k), 2 * (i * k + r * j), 2 * (i * j + r * k),
                     1 - 2 * (i * i + k * k), 2 * (j * k - r * i), 2 * (i * k - r * j), 2 * (j * k + r * i),
                     1 - 2 * (i * i + j * j)], 1).reshape(-1, 3, 3)
    inv = (R / (s * s)[:, None, :]) @ R.transpose(1, 2)
    axis = torch.linspace(-1, 1, RES).to(xyz.device)
    split, grow = RES // NB, 2 / NB * RELAX
    lo, hi = axis[::split] - grow, axis[split - 1::split] + grow
    cell = (torch.searchsorted(axis, pts.contiguous(), right=True) - 1).clamp(0, RES - 1) // split
    flat = (cell[:, 0] * NB + cell[:, 1]) * NB + cell[:, 2]
    density, G, col = torch.zeros(len(pts), device=xyz.device), torch.zeros_like(pts), torch.zeros_like(pts)
    for b in torch.unique(flat).tolist():
        bx, by, bz = b // (NB * NB), b // NB % NB, b % NB
        m = ((x[:, 0] > lo[bx]) & (x[:, 0] < hi[bx]) & (x[:, 1] > lo[by]) & (x[:, 1] < hi[by]) & (x[:, 2] > lo[bz]) & (x[:, 2] < hi[bz]))
        sel = (flat == b).nonzero().reshape(-1)
        if not m.any():
            continue
        d = pts[sel][:, None, :] - x[m][None]
        t = torch.einsum("gab,pgb->pga", inv[m], d)
        power = -0.5 * (t * d).sum(-1)
        w = o[m][None] * torch.where(power > 0, torch.zeros_like(power), torch.exp(power))
        density[sel] = w.sum(1)
        G[sel] = (w[..., None] * t).sum(1)
        col[sel] = w @ c[m]
    return density, torch.nn.functional.normalize(G, dim=1), col / density.clamp_min(1e-38)[:, None]


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip()
        return head + ("+changes" if dirty else "")
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_sample.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    from humangaussian_amd import _lib
    from humangaussian_amd.fields import GaussianField, marching_cubes
    if not torch.cuda.is_available():
        raise SystemExit("field_sample_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    cloud = tuple(torch.as_tensor(t, device=dev) for t in avatar(P, 1))
    colors = torch.as_tensor(np.random.default_rng(2).uniform(0, 1, (P, 3)).astype(np.float32), device=dev)
    with torch.no_grad():
        field = GaussianField(cloud, RES, NB, RELAX)
        v, f = marching_cubes(field.occ, 1.0)
        pts = (v / (RES - 1.0) * 2 - 1).contiguous()
        counts = field.block_counts.reshape(-1).long()
        axis = torch.linspace(-1, 1, RES).to(dev)
        cell = (torch.searchsorted(axis, pts, right=True) - 1).clamp(0, RES - 1) // (RES // NB)
        flat = (cell[:, 0] * NB + cell[:, 1]) * NB + cell[:, 2]
        sample_pairs = int(counts[flat].sum().item())
        field_pairs = int(counts.sum().item()) * (RES // NB) ** 3
        doc = {"_commit": a.commit or commit_id(), "_tool": "tools/field_sample_bench.py", "device": torch.cuda.get_device_name(0),
               "torch": torch.__version__, "gaussians": P, "resolution": RES, "num_blocks": NB, "vertices": int(len(pts)),
               "triangles": int(len(f)), "list_entries": int(counts.sum().item()), "fullest_list": int(counts.max().item()),
               "blocks_with_points": int(len(torch.unique(flat)))}
        doc["sample"] = entry(windows(lambda: field.sample(pts, colors, normalized=True), REPS), REPS, sample_pairs)
        doc["sample_without_colors"] = entry(windows(lambda: field.sample(pts, None, normalized=True), REPS), REPS, sample_pairs)
        print("sample", doc["sample"], flush=True)
        # hgs_field_eval alone, on the plan and the lists the field holds (it rebuilds the lists and rewrites occ: same bits)
        lib = _lib.load()
        info, ax, plan, lists = field._state
        occ = torch.empty_like(field.occ)
        info_buf = (ctypes.c_uint8 * 72).from_buffer_copy(info.numpy().tobytes())
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def run_eval():
            rc = lib.hgs_field_eval(ctypes.addressof(info_buf), ax.data_ptr(), plan.data_ptr(), lists.data_ptr(), occ.data_ptr(),
                                    None, stream)
            assert rc == 0, rc

        doc["field_eval"] = entry(windows(run_eval, REPS), REPS, field_pairs)
        assert torch.equal(occ.view(torch.int32), field.occ.view(torch.int32))
        print("field_eval", doc["field_eval"], flush=True)
        doc["sample_over_field_eval_pair_rate"] = doc["sample"]["pairs_per_s"] / doc["field_eval"]["pairs_per_s"]
        got = field.sample(pts, colors, normalized=True)
        ref = torch_blocks(cloud, field.center, field.scale, pts, colors)
        scale = ref[0].max().item()
        doc["max_abs_diff_vs_torch_blocks"] = {"density": (got[0] - ref[0]).abs().max().item(), "density_max": scale,
                                               "normal": (got[1] - ref[1]).abs().max().item(),
                                               "color": (got[2] - ref[2]).abs().max().item()}
        doc["torch_blocks"] = entry(windows(lambda: torch_blocks(cloud, field.center, field.scale, pts, colors), REPS_TORCH, 1),
                                    REPS_TORCH, sample_pairs)
        print("torch_blocks", doc["torch_blocks"], flush=True)
        doc["torch_blocks_over_sample"] = doc["torch_blocks"]["device_us_per_call"] / doc["sample"]["device_us_per_call"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
