"""Device time of drawing the pose-control images of one training step - B = 8 views at 512 x 512, fp32 - for both
styles:

  hip     humangaussian_amd.pose_image.PoseSkeleton.draw_views (one HIP launch per call: csrc/pose.hip)
  fill    torch's `zero_()` of a buffer of the same size: what this box takes to WRITE the same bytes and nothing else

Not part of bench.py.  The reference's path (per view: mvp to the host, cv2 on the CPU, upload) is not measured: cv2 and
seaborn are not installed on this stack, so there is no CPU number to compare against, only the byte floor.  Every style
is a child process of its own under its own time limit; after a child that crashed or ran out of time nothing more is
started.

Per measurement: WINDOWS windows of REPS warm calls each, device events around a window / REPS = `device_us_per_call`
(what the GPU's stream took, launch gaps included: where it equals `host_enqueue_us_per_call`, the host's enqueue time
bounds the window and the kernel itself is shorter - its own time is in a rocprofv3 kernel trace, a run of its own), hip
and fill windows alternating; medians over the windows, with the spread.  `bytes_written` = image + kp + records;
`bytes_per_s` = bytes_written / device time; `share_of_fill_rate` = the fill's device time / the call's; `share_of_copy_ceiling` = bytes_per_s / 6.29 TB/s, the float4 copy rate the project's other
tools use (a copy reads as much as it writes, so a pure write can exceed it).

    python tools/pose_image_bench.py [--out profiles/pose_image.json] [--commit ID]
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

B, H, W = 8, 512, 512
STYLES = ("openpose", "humansd")
COPY_CEILING = 6.29e12
WARMUP, WINDOWS, REPS = 50, 5, 500
CHILD_LIMIT_S = 180


def child(style):
    import numpy as np
    import torch
    import pose_reference as pr
    from humangaussian_amd import _lib
    from humangaussian_amd import pose_image as pi
    if not torch.cuda.is_available():
        raise SystemExit("pose_image_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    points = pr.make_skeleton(style, 0)
    rng = np.random.default_rng(1)
    mvp = np.stack([pr.orbit_mvp(rng.uniform(-30, 30), (rng.uniform() + i) / B * 360.0 - 180.0, rng.uniform(1.5, 2.0),
                                 rng.uniform(40, 70), H, W) for i in range(B)]).astype(np.float32)
    sk = pi.PoseSkeleton(points, humansd_style=style == "humansd", device=dev)
    m = torch.from_numpy(mvp).to(dev)
    image, kp, records = sk.draw_views(m, H, W, return_records=True)
    # the timed call computes what the tests check: the image of the records, and something is drawn
    want = torch.from_numpy(pr.to_float(pr.rasterise_batch(records.cpu().numpy(), H, W))).to(dev)
    assert torch.equal(image, want) and int((image != 0).sum()) > 0
    nbytes = image.numel() * 4 + kp.numel() * 4 + records.numel() * 4
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    binding = _lib.load_binding()
    style_id, width = (pi.HUMANSD, pi.default_limb_width(H)) if style == "humansd" else (pi.OPENPOSE, 1)
    run = {"hip": lambda: binding.pose_draw(sk.points3D, m, None, style_id, H, W, width, False),     # what draw_views calls
           "fill": lambda: scratch.zero_()}
    for _ in range(WARMUP):
        run["hip"]()
        run["fill"]()
    torch.cuda.synchronize()
    us = {"hip": [], "fill": []}
    host = {"hip": [], "fill": []}
    for _ in range(WINDOWS):
        for which in ("hip", "fill"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(REPS):
                run[which]()
            host[which].append((time.perf_counter() - t0) * 1e6 / REPS)
            e1.record()
            torch.cuda.synchronize()
            us[which].append(e0.elapsed_time(e1) * 1e3 / REPS)
    call, fill = statistics.median(us["hip"]), statistics.median(us["fill"])
    live = int((records[:, :, 0] != 0).sum())
    print(json.dumps({"style": style, "views": B, "height": H, "width": W, "records_drawn": live,
                      "device_us_per_call": call, "device_us_per_call_min_max": [min(us["hip"]), max(us["hip"])],
                      "host_enqueue_us_per_call": statistics.median(host["hip"]), "fill_host_enqueue_us": statistics.median(host["fill"]),
                      "fill_device_us": fill, "fill_device_us_min_max": [min(us["fill"]), max(us["fill"])],
                      "bytes_written": nbytes, "bytes_per_s": nbytes / (call * 1e-6), "share_of_fill_rate": fill / call,
                      "share_of_copy_ceiling": nbytes / (call * 1e-6) / COPY_CEILING,
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_image.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--child", metavar="STYLE")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    doc = {"_commit": a.commit or commit_id(), "_tool": "tools/pose_image_bench.py", "copy_ceiling_bytes_per_s": COPY_CEILING,
           "_note": "device time of one draw_views call; the reference's CPU path (cv2) cannot run on this stack and is not "
                    "measured - the comparison is against the bytes written",
           "styles": {}}
    for style in STYLES:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", style], capture_output=True, text=True,
                                 timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{style}: no result within {CHILD_LIMIT_S} s - stopping", file=sys.stderr)
            return 124
        if res.returncode != 0:
            print(f"{style}: exit status {res.returncode} - stopping\n{res.stderr[-2000:]}", file=sys.stderr)
            return res.returncode if res.returncode > 0 else 1
        doc["styles"][style] = json.loads(res.stdout.strip().splitlines()[-1])
        print(style, doc["styles"][style], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
