"""Device time of the surface sampler and of the initial Gaussians, N = 100 000 on the body mesh (`synth.human_mesh()`: the
reference's human.obj where the local asset exists, the capsule otherwise), in ONE run:

  sample              `SurfaceSampler.sample(N, return_anchors=True)`: hgs_surface_sample, one launch (points, face, uvw)
  sample_soup_20908_faces   the same call on a triangle soup of SMPL-X's face count (the table the kernel's staging is sized for)
  sample_torch        the same formulas as torch ops on the same GPU: torch.rand, torch.searchsorted on the same fp64 table,
                      the fold with torch.where, three gathers and the weighted sum (another generator: other samples)
  fill                a plain fill of the bytes a call writes (N x 28: points, face, uvw)
  build               `SurfaceSampler(vertices, faces)`: the table, with its one host wait (host clock, not device events)
  create              `create_from_points(points)`: distCUDA2 + hgs_init_gaussians, SH degree 0 and 3
  create_torch        the reference's chain (gaussian_model.py:127-147) as torch ops around the same distCUDA2
  dist2               distCUDA2 alone: what both forms of `create` share

Not part of bench.py.  Per measurement: WINDOWS windows of REPS warm calls each, device events around a window / REPS =
microseconds per call (what the GPU's stream took, launch gaps included); the median over the windows with their min and max.

    python tools/surface_sample_bench.py [--out profiles/surface_sample.json] [--commit ID]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 100_000
SMPLX_FACES = 20_908
WARMUP, WINDOWS, REPS = 20, 5, 200
C0 = 0.28209479177387814


def windows(run, reps=REPS):
    """-> microseconds per call for each window"""
    for i in range(WARMUP):
        run(i)
    torch.cuda.synchronize()
    out = []
    for w in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            run(WARMUP + w * reps + i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return out


def entry(us, nbytes=None):
    med = statistics.median(us)
    e = {"device_us_per_call": med, "device_us_per_call_min_max": [min(us), max(us)], "reps": REPS, "windows": WINDOWS}
    if nbytes is not None:
        e["bytes_written_per_call"] = nbytes
        e["bytes_per_s"] = nbytes / (med * 1e-6)
    return e


def sample_torch(v, f, table, n, gen):
    """trimesh.sample.sample_surface with the sampler's integer-free formulas, as torch ops"""
    r = torch.rand(n, 3, device=v.device, generator=gen)
    t = r[:, 0].double() * table[-1]
    face = torch.searchsorted(table, t, right=True).clamp_max(f.shape[0] - 1)
    k1, k2 = r[:, 1], r[:, 2]
    fold = k1 + k2 > 1.0
    k1, k2 = torch.where(fold, 1.0 - k1, k1), torch.where(fold, 1.0 - k2, k2)
    tri = f[face].long()
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    uvw = torch.stack([1.0 - k1 - k2, k1, k2], 1)
    return (a * uvw[:, 0:1] + b * uvw[:, 1:2]) + c * uvw[:, 2:3], face.int(), uvw


def create_torch(points, degree, distCUDA2):
    """gaussian_model.py:127-147 on a device tensor, colour 0.5"""
    P = points.shape[0]
    fused_color = (torch.full((P, 3), 0.5, device=points.device) - 0.5) / C0
    features = torch.zeros((P, 3, (degree + 1) ** 2), device=points.device)
    features[:, :3, 0] = fused_color
    features[:, 3:, 1:] = 0.0
    dist2 = torch.clamp_min(distCUDA2(points), 0.0000001)
    scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
    rots = torch.zeros((P, 4), device=points.device)
    rots[:, 0] = 1
    x = 0.1 * torch.ones((P, 1), dtype=torch.float, device=points.device)
    opacities = torch.log(x / (1 - x))
    return (features[:, :, 0:1].transpose(1, 2).contiguous(), features[:, :, 1:].transpose(1, 2).contiguous(), scales, rots,
            opacities, torch.zeros((P,), device=points.device))


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip()
        return head + ("+changes" if dirty else "")
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_sample.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_sample_bench: no GPU (a timing taken anywhere else says nothing)")
    from humangaussian_amd import surface, synth
    from humangaussian_amd.knn import distCUDA2
    dev = torch.device("cuda")
    mv, mf, label = synth.human_mesh()
    v, f = torch.as_tensor(mv, device=dev), torch.as_tensor(mf, device=dev)
    t0 = []
    for _ in range(5):
        torch.cuda.synchronize()
        s = time.perf_counter()
        sampler = surface.SurfaceSampler(v, f)
        t0.append((time.perf_counter() - s) * 1e6)
    doc = {"_commit": a.commit or commit_id(), "_tool": "tools/surface_sample_bench.py", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "N": N, "mesh": {"source": label, "vertices": int(v.shape[0]), "faces": int(f.shape[0])},
           "build": {"host_us_per_call_min_of_5": min(t0), "note": "table build + the one host wait, host clock"}}
    table = sampler.cdf
    gen = torch.Generator(device=dev).manual_seed(0)
    out_bytes = N * 28
    buf = torch.empty(out_bytes // 4, dtype=torch.float32, device=dev)
    with torch.no_grad():
        doc["sample"] = entry(windows(lambda i: sampler.sample(N, seed=1, offset=i * N, return_anchors=True)), out_bytes)
        doc["sample_points_only"] = entry(windows(lambda i: sampler.sample(N, seed=1, offset=i * N)), N * 12)
        doc["sample_torch"] = entry(windows(lambda i: sample_torch(v, f, table, N, gen)), out_bytes)
        doc["fill"] = entry(windows(lambda i: buf.fill_(1.0)), out_bytes)
        doc["sample_over_fill"] = doc["sample"]["device_us_per_call"] / doc["fill"]["device_us_per_call"]
        doc["sample_torch_over_sample"] = doc["sample_torch"]["device_us_per_call"] / doc["sample"]["device_us_per_call"]
        print({k: doc[k] for k in ("sample", "sample_points_only", "sample_torch", "fill")}, flush=True)
        # the table at SMPL-X's size (20 908 faces, 167 KB: 1 307 entries staged per workgroup), on a triangle soup
        g = torch.Generator().manual_seed(0)
        sv = (torch.rand(3 * SMPLX_FACES, 3, generator=g) * 2.0 - 1.0).to(dev)
        big = surface.SurfaceSampler(sv, torch.arange(3 * SMPLX_FACES, dtype=torch.int32, device=dev).reshape(-1, 3))
        doc["sample_soup_20908_faces"] = entry(windows(lambda i: big.sample(N, seed=1, offset=i * N, return_anchors=True)), out_bytes)
        print(doc["sample_soup_20908_faces"], flush=True)
        pts = sampler.sample(N, seed=1)
        doc["dist2"] = entry(windows(lambda i: distCUDA2(pts)))
        for degree in (0, 3):
            M = (degree + 1) ** 2
            nbytes = N * 4 * (3 * M + 3 + 4 + 1 + 1)
            hip = entry(windows(lambda i: surface.create_from_points(pts, None, degree)), nbytes)
            ref = entry(windows(lambda i: create_torch(pts, degree, distCUDA2)), nbytes)
            doc[f"create_degree{degree}"], doc[f"create_torch_degree{degree}"] = hip, ref
            doc[f"create_torch_over_create_degree{degree}"] = ref["device_us_per_call"] / hip["device_us_per_call"]
            for k in ("create", "create_torch"):
                doc[f"{k}_degree{degree}"]["device_us_without_dist2"] = (doc[f"{k}_degree{degree}"]["device_us_per_call"]
                                                                        - doc["dist2"]["device_us_per_call"])
            print(degree, hip, ref, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
