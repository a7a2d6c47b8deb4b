"""Do A/B builds of the library give the same bits?  Fingerprints (sha1 of every output, of the saved state and of every
gradient) of
  * forward + backward through the raw ABI on two single-view scenes (a small cloud with lists > 1024 entries: segments,
    transmittance products; a wider one), and
  * one batched call of 3 views of the small cloud through rasterize_gaussians_batch, forward + backward: the path of
    calls of >= 3 views (hgs_k_sort_lds_ch, chunk-cell-major pair rows, hgs_k_pair_reduce_ch) that no single-view call takes, and
  * the index builders beside the rasterizer, through the Python API (--save / --against only): distCUDA2 of a 100k-point
    cloud, mesh build + query on the 20,480-face icosphere, the 64^3 density field of an avatar cloud in 16 blocks, marching
    cubes of that field, prune_rows of 70,001 rows.

  python tools/cmp_variant.py variants/X/libhgs_rast.so [...]   raw-ABI cases: the in-tree build against every library given
  python tools/cmp_variant.py --save FILE                       all cases of THIS tree's build -> FILE (json)
  python tools/cmp_variant.py --against FILE                    all cases of this tree's build compared with a saved FILE

The torch binding finds its library by rpath, so the batched case cannot be pointed at another library inside one process:
build the other commit in its own checkout, --save there, --against here (each run a fresh process).  (On the GPU box.)"""
import argparse
import hashlib
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import torch
from abi_runner import RawCall
from helpers import make_scene
from humangaussian_amd import _lib

LONG = dict(P=2600, H=32, W=32, spread=0.02, scale=0.01, dist=2.0)


def h(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:12]


def fingerprint():
    out = []
    for name, kw, op in (("long", dict(seed=77, **LONG), 0.03),
                         ("wide", dict(P=6000, seed=5, H=128, W=160, spread=0.3, scale=0.05), None)):
        sc = make_scene(**kw)
        if op is not None:
            sc["opacities"] = torch.full_like(sc["opacities"], op)
        rc = RawCall(sc, capacity=1 << 18)
        assert rc.forward() == 0, rc.status
        out.append((name, "status", tuple(rc.status[:4]) + tuple(rc.status[6:8])))
        out.append((name, "outputs", h(rc.color), h(rc.depth), h(rc.alpha), h(rc.radii), h(rc.img)))
        g = torch.Generator().manual_seed(1)
        gc, gd, ga = (torch.randn(s, generator=g) for s in ((3, rc.H, rc.W), (1, rc.H, rc.W), (1, rc.H, rc.W)))
        grads = rc.backward(gc, gd, ga)
        out.append((name, "grads") + tuple(h(v) for v in grads.values() if v is not None))
    return out


def fingerprint_batch():
    """3 views of the "long" cloud in one call (cameras of make_scene seeds 77, 78, 79), every view with its own gradients"""
    from humangaussian_amd import GaussianRasterizationSettings, rasterize_gaussians_batch
    dev = "cuda"
    sc = make_scene(seed=77, **LONG)
    sc["opacities"] = torch.full_like(sc["opacities"], 0.03)
    cams = [make_scene(seed=s, **LONG)["cam"] for s in (77, 78, 79)]
    rsl = [GaussianRasterizationSettings(c.image_height, c.image_width, math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5),
                                         sc["bg"].to(dev), 1.0, c.world_view_transform.to(dev), c.full_proj_transform.to(dev),
                                         sc["sh_degree"], c.camera_center.to(dev), False, False) for c in cams]
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    ins = {k: sc[k].to(dev).requires_grad_(True) for k in names}
    B, P, H, W = len(cams), LONG["P"], LONG["H"], LONG["W"]
    m2 = torch.zeros(B, P, 3, device=dev, requires_grad=True)
    c, r, d, a = rasterize_gaussians_batch(ins["means3D"], m2, ins["shs"], None, ins["opacities"], ins["scales"],
                                           ins["rotations"], None, rsl)
    g = torch.Generator().manual_seed(1)
    gc, gd, ga = (torch.randn(s, generator=g).to(dev) for s in ((B, 3, H, W), (B, 1, H, W), (B, 1, H, W)))
    torch.autograd.backward([c, d, a], [gc, gd, ga])
    return [("batch3", "outputs", h(c), h(d), h(a), h(r)),
            ("batch3", "grads") + tuple(h(ins[k].grad) for k in names) + (h(m2.grad),)]


def fingerprint_index():
    """The k-NN grid, the mesh index, the density field, marching cubes and row compaction on fixed seeds: every quantity
    they produce is an integer or comes from the same fp32 operations in any build that computes the same thing."""
    import numpy as np
    import mesh_reference as R
    from humangaussian_amd import densify, synth
    from humangaussian_amd.fields import extract_fields, marching_cubes
    from humangaussian_amd.mesh import MeshIndex
    from simple_knn._C import distCUDA2
    dev = "cuda"
    out = []
    g = torch.Generator().manual_seed(3)
    out.append(("knn", "distCUDA2_100k", h(distCUDA2((torch.randn(100_000, 3, generator=g) * 0.4).to(dev)))))
    v, f = R.icosphere(5)
    idx = MeshIndex(v, f)
    rng = np.random.default_rng(4)
    pts = torch.as_tensor(rng.uniform(-1.3, 1.3, (20_000, 3)).astype(np.float32), device=dev)
    d, fc, uvw = idx.signed_distance(pts, return_uvw=True, mode="raystab")
    out.append(("mesh", "icosphere5", tuple(int(x) for x in idx.grid_dims), int(idx.num_refs), h(d), h(fc), h(uvw)))
    n = 20_000
    rng = np.random.default_rng(4)
    cloud = (synth.humanoid_points(n, seed=4).astype(np.float32), (0.002 + 0.95 * rng.uniform(size=(n, 1))).astype(np.float32),
             (0.012 * np.exp(0.5 * rng.normal(size=(n, 3)))).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32))
    res = extract_fields(tuple(torch.as_tensor(a, device=dev) for a in cloud), 64, 16, return_block_counts=True)
    occ, counts = res[0], res[-1]
    out.append(("field", "avatar_64_16", h(occ), h(counts)))
    mv, mt = marching_cubes(occ, 1.0)
    out.append(("mc", "avatar_64_16", tuple(mv.shape), tuple(mt.shape), h(mv), h(mt)))
    P = 70_001
    g = torch.Generator().manual_seed(2)
    keep = (torch.rand(P, generator=g) < 0.6).to(dev)
    rows = densify.prune_rows(keep, [torch.randn(P, 3, generator=g).to(dev), torch.randn(P, generator=g).to(dev)])
    out.append(("prune_rows", "70001") + tuple(h(r) for r in rows))
    return out


def report(label, ref, got):
    ok = got == ref
    print(label, "IDENTICAL" if ok else "DIFFERENT")
    if not ok:
        for a, b in zip(ref, got):
            if a != b:
                print("  ", a, "\n  ", b)
    return ok


def plain(fp):
    return json.loads(json.dumps(fp))          # (tuples -> lists: what a saved file holds)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", metavar="FILE")
    ap.add_argument("--against", metavar="FILE")
    ap.add_argument("libs", nargs="*")
    args = ap.parse_args()
    ref = fingerprint()
    for r in ref:
        print("in-tree", r)
    same = True
    if args.save or args.against:
        assert not args.libs, "library paths go with the raw-ABI mode only"
        allfp = plain(ref + fingerprint_batch() + fingerprint_index())
        for r in allfp[len(ref):]:
            print("in-tree", tuple(r))
        if args.save:
            with open(args.save, "w") as f:
                json.dump(allfp, f, indent=1)
        if args.against:
            with open(args.against) as f:
                same = report(args.against, json.load(f), allfp)
    for path in args.libs:
        _lib._lib = None
        _lib.LIB_PATH = os.path.abspath(path)
        same = report(path, ref, fingerprint()) and same
    sys.exit(0 if same else 1)
