"""Device time of the mesh view (humangaussian_amd/mesh_view.py, csrc/meshview.hip) on a body mesh of about SMPL-X's size -
`synth.humanoid_mesh(48, 36)`: 10 368 vertices, 20 160 faces - seen by the reference's orbit camera (radius 2, fovy 50), at
800 x 800 and 1024 x 1024, B = 1 and B = 8 views, in ONE run:

  render_normals     `MeshView.render_normals`: the whole call - normals, plan, the one host read, fill + draw (fused shading)
  rasterize          `MeshView.rasterize`: plan, host read, fill + draw writing rast
  stage_normals      hgs_meshview_normals alone (raw ABI, no host wait): hgs_k_mv_normals
  stage_plan         hgs_meshview_plan alone: two memsets, hgs_k_mv_vertex, hgs_k_mv_count, hgs_k_mv_scan1..3
  stage_draw         hgs_meshview_draw alone on a finished plan: hgs_k_mv_fill + hgs_k_mv_draw (the cursors are reset by a
                     device copy in front of every call; `stage_draw_reset` is that copy alone)
  stage_interpolate  hgs_meshview_interpolate on a stored rast
  fill               a plain fill of the bytes render_normals writes (B x H x W x 3 floats)
  normals_torch      the reference's vertex normals (animation.py:573-590: three scatter_add_, where, normalise) as torch ops
  render_frame       `AvatarAnimator.render_frame` of the same frame: 100 000 Gaussians anchored on the same mesh (B = 1)

Not part of bench.py.  Per measurement: WINDOWS windows of REPS warm calls each, device events around a window / REPS =
microseconds per call (what the GPU's stream took, launch gaps and - for the two whole calls - the host read included); the
median over the windows with their min and max.  `host_us_per_call` of the whole calls is the host clock around one call
that ends in a synchronise.  Kernel by kernel: rocprofv3 --kernel-trace --stats on this tool, in a run of its own.

    python tools/mesh_view_bench.py [--out profiles/mesh_view.json] [--commit ID]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARMUP, WINDOWS, REPS = 10, 5, 100
SIZES = (800, 1024)
VIEWS = (1, 8)
CLOUD = 100_000


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


def host_us(run, n=20):
    ts = []
    for i in range(n):
        torch.cuda.synchronize()
        s = time.perf_counter()
        run(i)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - s) * 1e6)
    return statistics.median(ts)


def entry(us, nbytes=None, **more):
    med = statistics.median(us)
    e = {"device_us_per_call": med, "device_us_per_call_min_max": [min(us), max(us)], "reps": REPS, "windows": WINDOWS}
    if nbytes is not None:
        e["bytes_written_per_call"] = nbytes
        e["bytes_per_s"] = nbytes / (med * 1e-6)
    e.update(more)
    return e


def normals_torch(vertices, faces):
    """animation.py:573-590"""
    i0, i1, i2 = faces[:, 0].long(), faces[:, 1].long(), faces[:, 2].long()
    v0, v1, v2 = vertices[i0, :], vertices[i1, :], vertices[i2, :]
    fn = torch.cross(v1 - v0, v2 - v0, dim=-1)
    vn = torch.zeros_like(vertices)
    vn.scatter_add_(0, i0[:, None].repeat(1, 3), fn)
    vn.scatter_add_(0, i1[:, None].repeat(1, 3), fn)
    vn.scatter_add_(0, i2[:, None].repeat(1, 3), fn)
    d = (vn * vn).sum(-1, keepdim=True)
    vn = torch.where(d > 1e-20, vn, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32, device=vn.device))
    return vn / torch.sqrt(torch.clamp((vn * vn).sum(-1, keepdim=True), min=1e-20))


class Cloud:
    """The reference GaussianModel's six tensors and getters: Gaussians on the mesh, random colours"""
    active_sh_degree = max_sh_degree = 0

    def __init__(self, xyz, spacing):
        P, dev = xyz.shape[0], xyz.device
        g = torch.Generator(device=dev).manual_seed(0)
        self._xyz = xyz
        self._features_dc = torch.randn(P, 1, 3, device=dev, generator=g) * 0.5
        self._features_rest = torch.zeros(P, 0, 3, device=dev)
        self._opacity = torch.full((P, 1), 2.0, device=dev)
        self._scaling = torch.full((P, 3), math.log(spacing), device=dev)
        self._rotation = torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(P, 1)

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


def stages(lib, view, v, mvp, H, W):
    """the raw ABI's stages, each timed alone on the current stream"""
    _lib = sys.modules["humangaussian_amd._lib"]
    dev = v.device
    B, V, F = mvp.shape[0], view.num_vertices, view.num_faces
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    records = torch.empty(B, V, 4, dtype=torch.int32, device=dev)
    plan = torch.empty(lib.hgs_meshview_plan_bytes(B, F, H, W), dtype=torch.uint8, device=dev)
    info_dev = torch.empty(32, dtype=torch.uint8, device=dev)
    normals = torch.empty(1, V, 3, device=dev)
    image = torch.empty(B, H, W, 3, device=dev)
    rast = torch.empty(B, H, W, 4, device=dev)
    a = _lib.HgsMeshviewArgs()
    a.B, a.V, a.F, a.H, a.W, a.C, a.shade_normals, a.background = B, V, F, H, W, 3, 1, 1.0
    a.vertices, a.mvp, a.faces = v.data_ptr(), mvp.data_ptr(), view.faces.data_ptr()
    a.adj_start, a.adj = view.adj_start.data_ptr(), view.adj.data_ptr()
    a.records, a.plan, a.info, a.normals, a.attr = records.data_ptr(), plan.data_ptr(), info_dev.data_ptr(), normals.data_ptr(), normals.data_ptr()
    ref = ctypes.byref(a)

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"mesh view stage failed with code {rc}")
    out = {"stage_normals": entry(windows(lambda i: check(lib.hgs_meshview_normals(ref, sp)))),
           "stage_plan": entry(windows(lambda i: check(lib.hgs_meshview_plan(ref, sp))))}
    torch.cuda.synchronize()
    info = _lib.HgsMeshviewInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    lists = torch.empty(max(lib.hgs_meshview_list_bytes(ctypes.byref(info)), 4), dtype=torch.uint8, device=dev)
    a.lists, a.image = lists.data_ptr(), image.data_ptr()
    saved = plan.clone()                      # the finished plan: a draw advances its cursors, so every call starts from a copy

    def draw(i):
        plan.copy_(saved)
        check(lib.hgs_meshview_draw(ref, ctypes.byref(info), sp))
    out["stage_draw"] = entry(windows(draw), B * H * W * 12)
    out["stage_draw_reset"] = entry(windows(lambda i: plan.copy_(saved)))
    a.image, a.rast = None, rast.data_ptr()
    draw(0)
    a.rast, a.rast_in, a.image, a.shade_normals = None, rast.data_ptr(), image.data_ptr(), 0
    out["stage_interpolate"] = entry(windows(lambda i: check(lib.hgs_meshview_interpolate(ref, sp))), B * H * W * 12)
    tiles = ((H + 15) // 16) * ((W + 15) // 16) * B
    out["list_entries"] = int(info.num_refs)
    out["tiles"] = tiles
    out["covered_share"] = float((rast[..., 3] > 0).float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_view.json"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_view_bench: no GPU (a timing taken anywhere else says nothing)")
    from humangaussian_amd import _lib, surface, synth
    from humangaussian_amd.animation import AvatarAnimator, orbit_frame_camera
    from humangaussian_amd.mesh_view import MeshView, mvp_from_camera
    dev = torch.device("cuda")
    lib = _lib.load()
    mv, mf = synth.humanoid_mesh(48, 36)
    v, f = torch.as_tensor(mv, device=dev), torch.as_tensor(mf, device=dev)
    view = MeshView(f, v.shape[0], device=dev)
    doc = {"_commit": args.commit or commit_id(), "_tool": "tools/mesh_view_bench.py", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "mesh": {"vertices": int(v.shape[0]), "faces": int(f.shape[0])},
           "list_batch": _lib.MESHVIEW_LIST_BATCH, "tile": _lib.MESHVIEW_TILE}
    with torch.no_grad():
        doc["normals"] = entry(windows(lambda i: view.vertex_normals(v)))
        doc["normals_torch"] = entry(windows(lambda i: normals_torch(v, f)))
        doc["normals_torch_over_normals"] = doc["normals_torch"]["device_us_per_call"] / doc["normals"]["device_us_per_call"]
        print({k: doc[k] for k in ("normals", "normals_torch")}, flush=True)
        pts = surface.SurfaceSampler(v, f).sample(CLOUD, seed=1)
        anim = AvatarAnimator.from_rest_pose(Cloud(pts, 0.004), mv, mf, white_background=True, device=dev)
        for S in SIZES:
            for B in VIEWS:
                cams = [orbit_frame_camera(45 * b, S, S, device=dev) for b in range(B)]
                mvp = torch.stack([mvp_from_camera(c) for c in cams]).to(dev).contiguous()
                nbytes = B * S * S * 12
                buf = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
                e = {"render_normals": entry(windows(lambda i: view.render_normals(v, mvp, S, S)), nbytes,
                                             host_us_per_call=host_us(lambda i: view.render_normals(v, mvp, S, S))),
                     "rasterize": entry(windows(lambda i: view.rasterize(v, mvp, S, S)), B * S * S * 16,
                                        host_us_per_call=host_us(lambda i: view.rasterize(v, mvp, S, S))),
                     "fill": entry(windows(lambda i: buf.fill_(1.0)), nbytes)}
                e.update(stages(lib, view, v, mvp, S, S))
                e["device_sum_of_stages_us"] = sum(e[k]["device_us_per_call"] for k in ("stage_normals", "stage_plan", "stage_draw")) \
                    - e["stage_draw_reset"]["device_us_per_call"]
                e["render_normals_over_fill"] = e["render_normals"]["device_us_per_call"] / e["fill"]["device_us_per_call"]
                if B == 1:
                    e["render_frame"] = entry(windows(lambda i: anim.render_frame(v, cams[0])), gaussians=int(anim.keep.sum()))
                    e["render_frame_over_render_normals"] = e["render_frame"]["device_us_per_call"] / e["render_normals"]["device_us_per_call"]
                doc[f"{S}x{S}_B{B}"] = e
                print(S, B, {k: (x["device_us_per_call"] if isinstance(x, dict) else x) for k, x in e.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
