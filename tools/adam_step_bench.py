"""Time of ONE optimizer step of the Gaussian model, for three optimizers on the same parameters and gradients:

  torch        torch.optim.Adam as the reference constructs it (gaussian_model.py:156-165: six groups of one tensor)
  torch_fused  torch.optim.Adam(fused=True), where the installed torch offers it on this device
  hip          humangaussian_amd.optim.GaussianAdam (one HIP launch for all groups)

at the shapes of BASELINE.json configs[1] (100k Gaussians, SH degree 0) and configs[3] (500k, SH degree 3).  Not part of
bench.py.  Every (shape, optimizer) measurement is a child process of its own under its own time limit; after a child
that crashed or ran out of time nothing more is started.

Per measurement: WINDOWS windows of REPS warm steps each.  `device_us` = device events around a window / REPS (what the
GPU's stream took per step, launch gaps included); `host_us` = host clock around the same calls WITHOUT a synchronise
(what the Python thread spent enqueueing a step).  Medians over the windows, with the spread.  `bytes` = 7 x 4 bytes per
element (param, grad and both moments read; param and both moments written); `share_of_copy_ceiling` = bytes /
device time / 6.29 TB/s (the measured float4 copy rate of the MI355X) - a whole-step rate, not a kernel's.

    python tools/adam_step_bench.py [--out profiles/adam_step.json] [--commit ID]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"configs1_100k_sh0": (100_000, 0), "configs3_500k_sh3": (500_000, 3)}
OPTIMIZERS = ("torch", "torch_fused", "hip")
LRS = {"xyz": 1.6e-4, "f_dc": 0.0025, "f_rest": 0.0025 / 20.0, "opacity": 0.05, "scaling": 0.005, "rotation": 0.001}
COPY_CEILING = 6.29e12
WARMUP, REPS, WINDOWS = 50, 200, 5
CHILD_LIMIT_S = 240


def shapes(P, deg):
    return {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, (deg + 1) ** 2 - 1, 3), "opacity": (P, 1), "scaling": (P, 3),
            "rotation": (P, 4)}


def child(shape_key, which):
    import torch
    from humangaussian_amd.optim import GaussianAdam
    if not torch.cuda.is_available():
        raise SystemExit("adam_step_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    P, deg = SHAPES[shape_key]
    g = torch.Generator().manual_seed(0)
    groups = []
    for name, shape in shapes(P, deg).items():
        p = torch.nn.Parameter(torch.randn(shape, generator=g).to(dev))
        p.grad = (torch.randn(shape, generator=g) * 0.1).to(dev)
        groups.append({"params": [p], "lr": LRS[name], "name": name})
    elems = sum(grp["params"][0].numel() for grp in groups)
    try:
        if which == "torch":
            opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        elif which == "torch_fused":
            opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=True)
        else:
            opt = GaussianAdam(groups, lr=0.0, eps=1e-15)
        opt.step()
        torch.cuda.synchronize()
    except Exception as e:                                  # fused=True where torch does not offer it
        if which != "torch_fused":
            raise
        print(json.dumps({"available": False, "why": f"{type(e).__name__}: {e}"[:300]}))
        return
    for _ in range(WARMUP):
        opt.step()
    torch.cuda.synchronize()
    dev_us, host_us = [], []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(REPS):
            opt.step()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        dev_us.append(e0.elapsed_time(e1) * 1e3 / REPS)
        host_us.append((t1 - t0) * 1e6 / REPS)
    nbytes = 7 * 4 * elems
    d = statistics.median(dev_us)
    print(json.dumps({"available": True, "device_us": d, "device_us_min_max": [min(dev_us), max(dev_us)],
                      "host_us": statistics.median(host_us), "host_us_min_max": [min(host_us), max(host_us)],
                      "elements": elems, "bytes": nbytes, "share_of_copy_ceiling": nbytes / (d * 1e-6) / COPY_CEILING,
                      "reps": REPS, "windows": WINDOWS, "device": torch.cuda.get_device_name(0), "torch": torch.__version__}))


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip()
        return head + ("+changes" if dirty else "")
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_step.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "OPTIMIZER"))
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return 0
    doc = {"_commit": a.commit or commit_id(), "_tool": "tools/adam_step_bench.py", "copy_ceiling_bytes_per_s": COPY_CEILING,
           "shapes": {}}
    for key in SHAPES:
        doc["shapes"][key] = {}
        for which in OPTIMIZERS:
            try:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, which], capture_output=True,
                                     text=True, timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f"{key} {which}: no result within {CHILD_LIMIT_S} s - stopping", file=sys.stderr)
                return 124
            if res.returncode != 0:
                print(f"{key} {which}: exit status {res.returncode} - stopping\n{res.stderr[-2000:]}", file=sys.stderr)
                return res.returncode if res.returncode > 0 else 1
            doc["shapes"][key][which] = json.loads(res.stdout.strip().splitlines()[-1])
            print(key, which, doc["shapes"][key][which], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
