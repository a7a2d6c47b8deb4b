"""Device time of the two re-anchoring passes and of the animation frame built on them, P = 100 000 Gaussians anchored on
the body mesh (`animation.human_mesh_anchors`), in ONE run:

  reanchor        hgs_reanchor (positions only: the reference's pass, animation.py:384-403)
  reanchor_rot    the pose form of hgs_reanchor_rot (positions + rotations carried by the anchor faces)
  frame_off/on    `AvatarAnimator.render_frame` at 1024 x 1024 (re-anchor + forward render) with repose_rotations off / on,
                  the posed vertices of eight `MotionDriver` frames computed beforehand, the camera of frame i

Not part of bench.py.  Per measurement: WINDOWS windows of REPS warm calls each, device events around a window / REPS =
microseconds per call (what the GPU's stream took, launch gaps included; the frame's host wait for its list length too);
the median over the windows with their min and max.  `bytes_per_call` = what a pass has to move once: per Gaussian the face
index, uvw and dist (20 B) and the position written (12 B), for the new pass also the rotation read and written (2 x 16 B);
the face and vertex tables once.  `bytes_per_s` = bytes_per_call / device time.

    python tools/reanchor_bench.py [--out profiles/reanchor_rot.json] [--commit ID] [--note TEXT]
"""
import argparse
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

P = 100_000
HW = 1024
WARMUP, WINDOWS = 20, 5
REPS_PASS, REPS_FRAME = 200, 40
POSES = 8


def windows(run, reps):
    """-> microseconds per call for each window"""
    n = 0
    for _ in range(WARMUP):
        run(n)
        n += 1
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run(n)
            n += 1
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return out


def entry(us, reps, nbytes=None):
    med = statistics.median(us)
    e = {"device_us_per_call": med, "device_us_per_call_min_max": [min(us), max(us)], "reps": reps, "windows": WINDOWS}
    if nbytes is not None:
        e["bytes_per_call"] = nbytes
        e["bytes_per_s"] = nbytes / (med * 1e-6)
    return e


class Model:
    """The reference GaussianModel's six tensors and getters (gaussian_model.py:95-115), SH degree 0"""
    active_sh_degree = max_sh_degree = 0

    def __init__(self, n, seed, device):
        rng = np.random.default_rng(seed)
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=device)  # noqa: E731
        self._xyz = torch.zeros(n, 3, device=device)
        self._features_dc, self._features_rest = t(rng.uniform(-1.5, 1.5, (n, 1, 3))), torch.zeros(n, 0, 3, device=device)
        self._opacity = t(rng.normal(0.0, 1.5, (n, 1)))
        self._scaling = t(np.log(0.004) + rng.normal(0.0, 0.4, (n, 1)) + np.log([[3.0, 1.0, 0.5]]))      # flat, elongated
        self._rotation = t(rng.standard_normal((n, 4)))

    get_xyz = property(lambda m: m._xyz)
    get_features = property(lambda m: torch.cat((m._features_dc, m._features_rest), dim=1))
    get_opacity = property(lambda m: torch.sigmoid(m._opacity))
    get_scaling = property(lambda m: torch.exp(m._scaling))
    get_rotation = property(lambda m: torch.nn.functional.normalize(m._rotation))


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip()
        return head + ("+changes" if dirty else "")
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reanchor_rot.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--note", default=None, help="recorded as `note` (e.g. why the new pass takes what it takes)")
    a = ap.parse_args()
    from humangaussian_amd import _lib
    from humangaussian_amd.animation import AvatarAnimator, MotionDriver, human_mesh_anchors, orbit_frame_camera
    if not torch.cuda.is_available():
        raise SystemExit("reanchor_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    binding = _lib.load_binding()
    rest, anchors = human_mesh_anchors(P, seed=0, device=dev)
    rest_t = torch.as_tensor(rest, device=dev)
    driver = MotionDriver(rest, device=dev)
    posed = [driver.vertices(3 + 17 * k).contiguous() for k in range(POSES)]
    model = Model(P, 1, dev)
    rot_base = anchors.bind_rotations(rest_t, model._rotation)
    tables = anchors.faces.numel() * 4 + rest_t.numel() * 4
    m = (anchors.faces, anchors.mapping_face, anchors.mapping_uvw, anchors.mapping_dist)

    doc = {"_commit": a.commit or commit_id(), "_tool": "tools/reanchor_bench.py", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "P": P, "mesh": {"vertices": int(rest_t.shape[0]), "faces": int(anchors.faces.shape[0])},
           "image": [HW, HW]}
    with torch.no_grad():
        old = windows(lambda i: binding.reanchor(posed[i % POSES], *m), REPS_PASS)
        new = windows(lambda i: binding.reanchor_rot(posed[i % POSES], *m, rot_base, False), REPS_PASS)
        # the two passes agree on the positions, bit for bit
        assert torch.equal(binding.reanchor(posed[0], *m).view(torch.int32),
                           binding.reanchor_rot(posed[0], *m, rot_base, False)[0].view(torch.int32))
        doc["reanchor"] = entry(old, REPS_PASS, P * 32 + tables)
        doc["reanchor_rot"] = entry(new, REPS_PASS, P * 64 + tables)
        doc["reanchor_rot_over_reanchor"] = doc["reanchor_rot"]["device_us_per_call"] / doc["reanchor"]["device_us_per_call"]
        print("reanchor", doc["reanchor"], "\nreanchor_rot", doc["reanchor_rot"], flush=True)
        cams = [orbit_frame_camera(i, HW, HW, device=dev) for i in range(POSES)]
        for name, on in (("frame_off", False), ("frame_on", True)):
            anim = AvatarAnimator(Model(P, 1, dev), anchors, white_background=True, device=dev, repose_rotations=on,
                                  rest_vertices=rest_t if on else None)
            us = windows(lambda i: anim.render_frame(posed[i % POSES], cams[i % POSES]), REPS_FRAME)
            doc[name] = entry(us, REPS_FRAME)
            print(name, doc[name], flush=True)
        doc["frame_on_minus_off_us"] = doc["frame_on"]["device_us_per_call"] - doc["frame_off"]["device_us_per_call"]
    if a.note:
        doc["note"] = a.note
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
