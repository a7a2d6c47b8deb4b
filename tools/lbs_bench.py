"""Time of posing a skinned body at SMPL-X size (V = 10 475, J = 55, K = 486; synthetic arrays), per frame, for

  hip          humangaussian_amd.body.SkinnedBody.pose (two HIP launches per call: csrc/lbs.hip)
  hip_cold     the same with the 61 MB table of pose blend shapes rotated over six copies (366 MB: more than the 256 MB
               Infinity Cache holds), so that every call streams its table from HBM
  torch        the same formulas written in torch ops on the same GPU (the `smplx` package's lbs(): batch_rodrigues, a
               matmul with posedirs, a Python loop over the kinematic chain, a matmul with the dense weights)

for calls of F = 1 and F = 136 frames.  Not part of bench.py.  Every (F, path) measurement is a child process of its own
under its own time limit; after a child that crashed or ran out of time nothing more is started.

Per measurement: WINDOWS windows of REPS warm calls each, device events around a window / REPS / F = `device_us_per_frame`
(what the GPU's stream took, launch gaps included); medians over the windows, with the spread.  `bytes_per_call` = what a
call has to move once: the table once per tile of frames (F = 1: one tile; else ceil(F / 8)), v_shaped and the packed
weights once per tile, the vertices written; `bytes_per_s` = bytes_per_call / device time of a call.

    python tools/lbs_bench.py [--out profiles/lbs_step.json] [--commit ID]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

V, J = 10475, 55
K = 9 * (J - 1)
FRAMES = (1, 136)
PATHS = ("hip", "hip_cold", "torch")
COPY_CEILING = 6.29e12
WARMUP, WINDOWS = 20, 5
REPS = {1: 200, 136: 20}
COLD_COPIES = 6
CHILD_LIMIT_S = 240


def synthetic_body(seed=0):
    import numpy as np
    from humangaussian_amd.body import SMPLX_PARENTS
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, (V, 3)).astype(np.float32)
    reg = rng.uniform(0.0, 1.0, (J, V)) ** 4
    w = np.zeros((V, J))
    for i in range(V):
        idx = rng.choice(J, size=4 if i == 0 else int(rng.integers(1, 5)), replace=False)
        w[i, idx] = rng.uniform(0.05, 1.0, idx.size)
    return dict(v_template=v, faces=np.zeros((0, 3), np.int32), parents=np.array(SMPLX_PARENTS, np.int32),
                J_regressor=(reg / reg.sum(1, keepdims=True)).astype(np.float32),
                weights=(w / w.sum(1, keepdims=True)).astype(np.float32),
                posedirs=(rng.standard_normal((K, 3 * V)) * 0.01).astype(np.float32))


def torch_lbs(t, poses):
    """lbs() in torch ops: poses (F, J, 3) -> vertices (F, V, 3)"""
    import torch
    F = poses.shape[0]
    a = poses.reshape(-1, 3)
    angle = torch.norm(a + 1e-8, dim=1, keepdim=True)
    k = a / angle
    zeros = torch.zeros_like(k[:, 0])
    Kx = torch.stack([zeros, -k[:, 2], k[:, 1], k[:, 2], zeros, -k[:, 0], -k[:, 1], k[:, 0], zeros], 1).view(-1, 3, 3)
    s, c = torch.sin(angle)[:, None], torch.cos(angle)[:, None]
    R = (t["eye"] + s * Kx + (1 - c) * torch.bmm(Kx, Kx)).view(F, J, 3, 3)
    pf = (R[:, 1:] - t["eye"]).reshape(F, K)
    v_posed = t["v_shaped"][None] + torch.matmul(pf, t["posedirs"]).view(F, V, 3)
    rel = t["rel"]
    top = torch.cat([R, rel[None].expand(F, J, 3)[..., None]], 3)
    M = torch.cat([top, t["bottom"].expand(F, J, 1, 4)], 2)                         # (F, J, 4, 4)
    chain = [M[:, 0]]
    for j in range(1, J):
        chain.append(torch.matmul(chain[t["parents_host"][j]], M[:, j]))
    G = torch.stack(chain, 1)
    Jh = torch.cat([t["J_rest"], t["J_rest"].new_zeros(J, 1)], 1)[None, :, :, None]
    A = G - torch.nn.functional.pad(torch.matmul(G, Jh), [3, 0])
    T = torch.matmul(t["weights"][None], A.view(F, J, 16)).view(F, V, 4, 4)
    vh = torch.cat([v_posed, v_posed.new_ones(F, V, 1)], 2)
    return (torch.matmul(T, vh[..., None])[:, :, :3, 0] - t["centre"]) * t["scale"]


def child(F, which):
    import numpy as np
    import torch
    from humangaussian_amd import _lib
    from humangaussian_amd.body import SkinnedBody
    if not torch.cuda.is_available():
        raise SystemExit("lbs_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    b = synthetic_body()
    sb = SkinnedBody(b["v_template"], b["faces"], b["parents"], b["J_regressor"], b["weights"], posedirs=b["posedirs"], device=dev)
    rng = np.random.default_rng(1)
    d = rng.standard_normal((F, J, 3))
    poses = torch.from_numpy((d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0, 1.0, (F, J, 1))).astype(np.float32)).to(dev)
    centre, scale = [0.01, -0.02, 0.03], 1.5
    reps = REPS[F]
    if which == "torch":
        t = dict(eye=torch.eye(3, device=dev), v_shaped=sb.v_shaped, J_rest=sb.J_rest, parents_host=[int(p) for p in b["parents"]],
                 posedirs=torch.from_numpy(b["posedirs"]).to(dev), weights=torch.from_numpy(b["weights"]).to(dev),
                 bottom=torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev).view(1, 1, 1, 4),
                 centre=torch.tensor(centre, device=dev), scale=scale)
        par = torch.as_tensor(b["parents"]).long().clamp(min=0).to(dev)
        t["rel"] = sb.J_rest - torch.where((torch.arange(J, device=dev) > 0)[:, None], sb.J_rest[par], torch.zeros_like(sb.J_rest))
        with torch.no_grad():
            run = lambda i: torch_lbs(t, poses)    # noqa: E731
            got, want = run(0), sb.pose(poses, centre=centre, scale=scale)
            agree = float((got - want).abs().max())
            assert agree < 1e-4, agree                                      # the two paths compute the same thing
    else:
        tables = [sb.posedirs] + ([sb.posedirs.clone() for _ in range(COLD_COPIES - 1)] if which == "hip_cold" else [])
        binding = _lib.load_binding()
        run = lambda i: binding.lbs_pose(sb.v_shaped, sb.J_rest, sb.parents, tables[i % len(tables)], sb.weight_joint,   # noqa: E731
                                         sb.weight_value, poses, None, centre, scale, False)
        agree = None
    n = 0
    for _ in range(WARMUP):
        run(n)
        n += 1
    torch.cuda.synchronize()
    dev_us = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run(n)
            n += 1
        e1.record()
        torch.cuda.synchronize()
        dev_us.append(e0.elapsed_time(e1) * 1e3 / reps)
    tiles = 1 if F == 1 else -(-F // _lib.LBS_FRAME_TILE)
    table = sb.posedirs.numel() * 4
    nbytes = tiles * (table + V * 12 + V * sb.weight_width * 8) + F * V * 12
    call = statistics.median(dev_us)
    print(json.dumps({"frames": F, "device_us_per_call": call, "device_us_per_frame": call / F,
                      "device_us_per_frame_min_max": [min(dev_us) / F, max(dev_us) / F], "table_bytes": table,
                      "bytes_per_call": nbytes, "bytes_per_s": nbytes / (call * 1e-6),
                      "share_of_copy_ceiling": nbytes / (call * 1e-6) / COPY_CEILING, "max_abs_diff_to_hip": agree,
                      "reps": reps, "windows": WINDOWS, "device": torch.cuda.get_device_name(0), "torch": torch.__version__}))


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip()
        return head + ("+changes" if dirty else "")
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbs_step.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--child", nargs=2, metavar=("FRAMES", "PATH"))
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), a.child[1])
        return 0
    doc = {"_commit": a.commit or commit_id(), "_tool": "tools/lbs_bench.py", "copy_ceiling_bytes_per_s": COPY_CEILING,
           "shape": {"V": V, "J": J, "K": K}, "frames": {}}
    for F in FRAMES:
        res_f = doc["frames"][f"F{F}"] = {}
        for which in PATHS:
            try:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(F), which], capture_output=True,
                                     text=True, timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f"F={F} {which}: no result within {CHILD_LIMIT_S} s - stopping", file=sys.stderr)
                return 124
            if res.returncode != 0:
                print(f"F={F} {which}: exit status {res.returncode} - stopping\n{res.stderr[-2000:]}", file=sys.stderr)
                return res.returncode if res.returncode > 0 else 1
            res_f[which] = json.loads(res.stdout.strip().splitlines()[-1])
            print(f"F={F}", which, res_f[which], flush=True)
        res_f["torch_over_hip"] = res_f["torch"]["device_us_per_frame"] / res_f["hip"]["device_us_per_frame"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
