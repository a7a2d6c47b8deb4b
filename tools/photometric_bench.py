"""Time of the photometric loss of image fitting, forward + backward (the loss at lambda_dssim = 0.2 and its gradient with
respect to the image), fp32, at 1 x 3 x 1024 x 1024 and 8 x 3 x 1024 x 1024, for

  hip      humangaussian_amd.photometric_loss and its backward (two HIP launches forward, one backward: csrc/photometric.hip)
  torch    the same formulas written in torch ops under autograd on the same GPU (what the reference's train.py runs: five
           depthwise 11 x 11 conv2d and the elementwise chain of _ssim, l1_loss, and their backward)
  copy     a plain device copy of as many bytes as `hip` has to move (see below), as the floor a streaming kernel can reach

Not part of bench.py.  Every (shape, path) is a child process of its own under its own time limit; after a child that
crashed or ran out of time nothing more is started.

Per path: WINDOWS windows of REPS warm calls each, device events around a window / REPS = `device_us_per_call` (what the
GPU's stream took, launch gaps included) and the host's time to enqueue a call; medians over the windows, with the spread.
`counted_bytes_per_call` is COUNTED, not measured: forward - image and gt read once, three derivative maps written; backward -
the three maps, image and gt read once, the gradient written: 13 fp32 values per element.  (The kernels read each tile
with its halo of 5, 1.7 x the tile, so `bytes_per_s` understates what they ask of the caches.)

    python tools/photometric_bench.py [--out profiles/photometric.json] [--commit ID]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"1x3x1024x1024": (1, 3, 1024, 1024), "8x3x1024x1024": (8, 3, 1024, 1024)}
PATHS = ("hip", "torch", "copy")
COPY_CEILING = 6.29e12
LAMBDA = 0.2
WARMUP, WINDOWS = 10, 5
REPS = {"hip": 50, "torch": 10, "copy": 50}
CHILD_LIMIT_S = 240


def counted_bytes(shape):
    n = shape[0] * shape[1] * shape[2] * shape[3]
    return (2 + 3 + 3 + 2 + 1) * n * 4


def inputs(shape, dev):
    import torch
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(shape, generator=g)
    image = (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0.0, 1.0)       # a fit under way: close to the photograph
    return image.to(dev), gt.to(dev)


def child(which, shape_name):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("photometric_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    shape = SHAPES[shape_name]
    image, gt = inputs(shape, dev)
    agree = None
    if which == "copy":
        src = torch.empty(counted_bytes(shape) // 2, dtype=torch.uint8, device=dev)     # a copy reads and writes every byte
        dst = torch.empty_like(src)
        run = lambda: dst.copy_(src)    # noqa: E731
    else:
        from humangaussian_amd import photometric_loss
        import photometric_reference as pr

        def hip(x):
            return photometric_loss(x, gt, LAMBDA).loss

        def ops(x):
            return pr.formulas(x, gt, LAMBDA)["loss"]
        leaf = image.clone().requires_grad_(True)      # the clone belongs to neither path: made outside the timed call
        fn = hip if which == "hip" else ops

        def run():
            leaf.grad = None
            fn(leaf).backward()
        if which == "torch":
            a, = torch.autograd.grad(hip(leaf), leaf)
            b, = torch.autograd.grad(ops(leaf), leaf)
            agree = float((a - b).abs().max() / b.abs().max())
            assert agree < 1e-4, agree                                      # the two paths compute the same thing
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    reps, dev_us, host_us = REPS[which], [], []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(reps):
            run()
        host_us.append((time.perf_counter() - t0) * 1e6 / reps)          # what the host took to enqueue a call
        e1.record()
        torch.cuda.synchronize()
        dev_us.append(e0.elapsed_time(e1) * 1e3 / reps)
    call = statistics.median(dev_us)
    nbytes = counted_bytes(shape)
    print(json.dumps({"device_us_per_call": call, "device_us_per_call_min_max": [min(dev_us), max(dev_us)],
                      "host_enqueue_us_per_call": statistics.median(host_us),
                      "counted_bytes_per_call": nbytes, "bytes_per_s": nbytes / (call * 1e-6),
                      "share_of_copy_ceiling": nbytes / (call * 1e-6) / COPY_CEILING, "max_rel_diff_of_gradient_to_hip": agree,
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--child", nargs=2, metavar=("PATH", "SHAPE"))
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return 0
    doc = {"_commit": a.commit or commit_id(), "_tool": "tools/photometric_bench.py", "copy_ceiling_bytes_per_s": COPY_CEILING,
           "what": "forward + backward of the loss at lambda_dssim = 0.2, fp32", "shapes": {}}
    for shape_name in SHAPES:
        paths = {}
        for which in PATHS:
            try:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, shape_name], capture_output=True,
                                     text=True, timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f"{shape_name} {which}: no result within {CHILD_LIMIT_S} s - stopping", file=sys.stderr)
                return 124
            if res.returncode != 0:
                print(f"{shape_name} {which}: exit status {res.returncode} - stopping\n{res.stderr[-2000:]}", file=sys.stderr)
                return res.returncode if res.returncode > 0 else 1
            paths[which] = json.loads(res.stdout.strip().splitlines()[-1])
            print(shape_name, which, paths[which], flush=True)
        doc["shapes"][shape_name] = {"paths": paths,
                                     "torch_over_hip": paths["torch"]["device_us_per_call"] / paths["hip"]["device_us_per_call"],
                                     "copy_over_hip": paths["copy"]["device_us_per_call"] / paths["hip"]["device_us_per_call"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
