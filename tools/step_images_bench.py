"""Time of the step's guidance images and opacity losses, forward + backward, at the training step's size (B = 8 views,
1024 x 1024 -> 512 x 512, fp32), for

  hip      humangaussian_amd.guidance_images and its backward with all four gradients (three HIP launches each way:
           csrc/step_images.hip)
  torch    the same formulas written in torch ops under autograd on the same GPU (what the reference's training step runs:
           amin / amax / max, the normalisation, two F.interpolate, the two losses, and their backward)
  copy     a plain device copy of as many bytes as `hip` has to move (see below), as the floor a streaming kernel can reach

Not part of bench.py.  Every path is a child process of its own under its own time limit; after a child that crashed or
ran out of time nothing more is started.

Per path: WINDOWS windows of REPS warm calls each, device events around a window / REPS = `device_us_per_call` (what the
GPU's stream took, launch gaps included) and the host's time to enqueue a call (`host_enqueue_us_per_call`: where it is
close to the device time, the path is bound by the host); medians over the windows, with the spread.  `bytes_per_call` is COUNTED, not
measured: forward - colour and depth read once, two (B, 3, h, w) images written; backward - the two image gradients read,
dL/dcolour and dL/ddepth written.  (The kernels read the depth more often than once - min / max, the losses and the
resize are three passes, the backward two - so `bytes_per_s` understates what they move.)

    python tools/step_images_bench.py [--out profiles/step_images.json] [--commit ID]
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

B, H, W, h, w = 8, 1024, 1024, 512, 512
PATHS = ("hip", "torch", "copy")
COPY_CEILING = 6.29e12
WARMUP, WINDOWS = 10, 5
REPS = {"hip": 50, "torch": 20, "copy": 50}
CHILD_LIMIT_S = 240


def counted_bytes():
    fwd = (B * 3 * H * W + B * H * W) * 4 + 2 * B * 3 * h * w * 4
    bwd = 2 * B * 3 * h * w * 4 + (B * 3 * H * W + B * H * W) * 4
    return fwd + bwd


def inputs(dev):
    import torch
    g = torch.Generator().manual_seed(0)
    render = torch.rand(B, 3, H, W, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    inside = (yy / 0.8) ** 2 + (xx / 0.45) ** 2 <= 1.0                      # about 70 % background, as a rendered body has
    depth = torch.where(inside, 1.0 + 1.5 * torch.rand(B, 1, H, W, generator=g), torch.zeros(()))
    grads = [torch.randn(B, 3, h, w, generator=g), torch.randn(B, 3, h, w, generator=g), torch.tensor(1.0), torch.tensor(0.25)]
    return render.to(dev), depth.to(dev), [t.to(dev) for t in grads]


def child(which):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("step_images_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    render, depth, grads = inputs(dev)
    agree = None
    if which == "copy":
        src = torch.empty(counted_bytes() // 2, dtype=torch.uint8, device=dev)     # a copy reads and writes every byte
        dst = torch.empty_like(src)
        run = lambda: dst.copy_(src)    # noqa: E731
    else:
        from humangaussian_amd import guidance_images
        import step_images_reference as sr

        def step(fn):
            r, d = render.clone().requires_grad_(True), depth.clone().requires_grad_(True)
            out = fn(r, d)
            torch.autograd.backward(list(out), grads)
            return r.grad, d.grad

        def hip(r, d):
            o = guidance_images(r, d, size=(h, w))
            return o.rgb, o.depth, o.loss_sparsity, o.loss_opaque

        def ops(r, d):
            o = sr.formulas(r, d, (h, w))
            return o["rgb"], o["depth"], o["loss_sparsity"], o["loss_opaque"]
        # the clones of the inputs belong to neither path: they are made outside the timed call
        r_leaf, d_leaf = render.clone().requires_grad_(True), depth.clone().requires_grad_(True)
        fn = hip if which == "hip" else ops

        def run():
            r_leaf.grad = d_leaf.grad = None
            torch.autograd.backward(list(fn(r_leaf, d_leaf)), grads)
        if which == "torch":
            a, b = step(hip), step(ops)
            agree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b)]
            assert max(agree) < 1e-4, agree                                 # the two paths compute the same thing
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
    nbytes = counted_bytes()
    print(json.dumps({"device_us_per_call": call, "device_us_per_call_min_max": [min(dev_us), max(dev_us)],
                      "host_enqueue_us_per_call": statistics.median(host_us),
                      "counted_bytes_per_call": nbytes, "bytes_per_s": nbytes / (call * 1e-6),
                      "share_of_copy_ceiling": nbytes / (call * 1e-6) / COPY_CEILING, "max_rel_diff_of_gradients_to_hip": agree,
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_images.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--child", metavar="PATH")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    doc = {"_commit": a.commit or commit_id(), "_tool": "tools/step_images_bench.py", "copy_ceiling_bytes_per_s": COPY_CEILING,
           "shape": {"B": B, "H": H, "W": W, "h": h, "w": w, "dtype": "float32"}, "what": "forward + backward, all four gradients",
           "paths": {}}
    for which in PATHS:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], capture_output=True, text=True,
                                 timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{which}: no result within {CHILD_LIMIT_S} s - stopping", file=sys.stderr)
            return 124
        if res.returncode != 0:
            print(f"{which}: exit status {res.returncode} - stopping\n{res.stderr[-2000:]}", file=sys.stderr)
            return res.returncode if res.returncode > 0 else 1
        doc["paths"][which] = json.loads(res.stdout.strip().splitlines()[-1])
        print(which, doc["paths"][which], flush=True)
    doc["torch_over_hip"] = doc["paths"]["torch"]["device_us_per_call"] / doc["paths"]["hip"]["device_us_per_call"]
    doc["hip_over_copy"] = doc["paths"]["hip"]["device_us_per_call"] / doc["paths"]["copy"]["device_us_per_call"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
