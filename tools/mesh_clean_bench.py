"""Device time of the mesh cleaning and decimation (csrc/meshclean.hip: mesh_components, clean_mesh, decimate_mesh) on the
raw iso-surface of the benchmark avatar: 100 000 Gaussians on the body cloud, resolutions 128 and 512.

  components        mesh_components(vertices, faces): the label rounds (a host read every four) + the per-component sums
  clean             clean_mesh(vertices, faces): the components, the keep rule, two compactions, the gathers
  decimate_100000   decimate_mesh to 100 000 faces (the reference's decimate_target) - a no-op where the mesh has fewer
  decimate_10000    decimate_mesh to 10 000 faces: the bisection (5 launches, 5 host reads), two hash tables, the means
  extract           extract_fields + marching_cubes of the same avatar: what the mesh cost to make, the yardstick
  copy_*            a device copy that moves as many bytes as the call reads and writes (its inputs and outputs once)

Not part of bench.py.  Per measurement WINDOWS windows of warm calls, device events around a window / reps = microseconds
per call (the calls' host reads lie inside the windows); the median over the windows with their min and max.  Nothing
here is a gate.

    python tools/mesh_clean_bench.py [--out profiles/mesh_clean.json] [--commit ID] [--resolutions 128 512]
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
WARMUP, WINDOWS = 3, 5
REPS = {128: 20, 512: 5}
REPS_EXTRACT = {128: 10, 512: 2}


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


def entry(us, reps, **extra):
    e = {"device_us_per_call": statistics.median(us), "device_us_per_call_min_max": [min(us), max(us)], "reps": reps,
         "windows": WINDOWS}
    e.update(extra)
    return e


def copy_entry(nbytes, reps, dev):
    """a device copy whose reads plus writes are nbytes"""
    half = max(int(nbytes) // 2, 1)
    src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
    return entry(windows(lambda: dst.copy_(src), reps), reps, bytes=int(nbytes))


def mesh_bytes(v, f):
    return int(v.shape[0]) * 12 + int(f.shape[0]) * 12


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip()
        return head + ("+changes" if dirty else "")
    except Exception:
        return "unknown"


def measure(cloud, res, dev):
    from humangaussian_amd.fields import extract_fields, marching_cubes
    from humangaussian_amd.meshclean import clean_mesh, decimate_mesh, mesh_components

    def extract():
        occ, center, scale = extract_fields(cloud, res)
        v, f = marching_cubes(occ, 1.0)
        return (v / (res - 1.0) * 2 - 1) / scale + center, f

    v, f = extract()
    reps = REPS[res]
    doc = {"resolution": res, "vertices": int(v.shape[0]), "faces": int(f.shape[0])}
    doc["extract"] = entry(windows(extract, REPS_EXTRACT[res], 1), REPS_EXTRACT[res])
    print(res, "extract", doc["extract"], flush=True)
    labels, comp_faces, _, rounds = mesh_components(v, f, return_rounds=True)
    doc["components"] = entry(windows(lambda: mesh_components(v, f), reps), reps, rounds=int(rounds),
                              components=int((labels == torch.arange(len(labels), device=dev)).sum()),
                              components_with_faces=int((comp_faces > 0).sum()))
    doc["copy_components"] = copy_entry(mesh_bytes(v, f) + 12 * v.shape[0], reps, dev)
    print(res, "components", doc["components"], flush=True)
    cv, cf = clean_mesh(v, f)
    doc["clean"] = entry(windows(lambda: clean_mesh(v, f), reps), reps, rounds=int(rounds), vertices_out=int(cv.shape[0]),
                         faces_out=int(cf.shape[0]))
    doc["copy_clean"] = copy_entry(mesh_bytes(v, f) + mesh_bytes(cv, cf), reps, dev)
    print(res, "clean", doc["clean"], flush=True)
    for target in (100_000, 10_000):
        dv, df, info = decimate_mesh(cv, cf, target, return_info=True)
        extra = {"vertices_in": int(cv.shape[0]), "faces_in": int(cf.shape[0]), "vertices_out": int(dv.shape[0]),
                 "faces_out": int(df.shape[0]), "no_op": info is None}
        if info is not None:
            extra.update(grid=info["grid"], cell=info["cell"], bisection_probes=10, probe_launches=info["probe_launches"])
        doc[f"decimate_{target}"] = entry(windows(lambda: decimate_mesh(cv, cf, target), reps), reps, **extra)
        doc[f"copy_decimate_{target}"] = copy_entry(mesh_bytes(cv, cf) + mesh_bytes(dv, df), reps, dev)
        print(res, "decimate", target, doc[f"decimate_{target}"], flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 512])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    cloud = tuple(torch.as_tensor(t, device=dev) for t in avatar(P, 1))
    doc = {"_commit": a.commit or commit_id(), "_tool": "tools/mesh_clean_bench.py", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "gaussians": P,
           "note": "decimate_* run on the cleaned mesh, as extract_clean_mesh(decimate_target=T) does; the calls' host "
                   "reads (component rounds: one per four rounds; bisection: one per launch; one for the output sizes) are "
                   "inside the windows"}
    with torch.no_grad():
        for res in a.resolutions:
            doc[f"resolution_{res}"] = measure(cloud, res, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
