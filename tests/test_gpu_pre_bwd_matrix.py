"""The per-Gaussian backward (`preprocess_bwd_body`, csrc/preprocess.hip) swept over its dispatch matrix against the fp64
oracle.  One template is compiled into 24 kernels - SH degree 0-3 x {loop over the views `d*`, one view `s*`, thread per
(Gaussian, view) `p*`} x {filter off, `_aa`} - picked by csrc/api.hip from (views, degree, antialiasing, LDS budget);
inside each an SH block travels one of three ways (staged through LDS, 16-byte vectors, scalars) or into the packed row.
Every output tensor is `at::empty`: what a path forgets to write is whatever the allocator held.

CASES is the table (plain data, importable without a GPU; tests/test_pre_bwd_matrix_cpu.py checks that it reaches every
kernel, SH path and boundary, and that its scenes are well conditioned).  Per case: all gradients finite, within
GRAD_TOL of max|g64| with cosine >= 1 - COS_TOL (the gates of tests/test_gpu_parity.py and tests/test_gpu_antialias.py),
the gradient of the inactive SH coefficients (M > (D+1)^2) bitwise zero, the packed row == `pack_contribution` of the
six tensors bitwise.  Then the relations that hold bit for bit (one write per element, fixed summation order,
-ffp-contract=off): padding M, batched == per-view calls summed in view order, and the loop form (a second build with
HGS_PRE_BWD_VPAR_MIN_VIEWS above HGS_MAX_VIEWS, the only way `d0`, `d1`, `d0_aa`, `d1_aa` run on a device that grants the
160 KB LDS raise) == the thread-per-(Gaussian, view) form.  Last, the fused activations' chain rule at the edges.

The reference is `oracle.forward_backward(dtype=float64)` (with the filter: tests/aa_reference.py) per (scene, view),
computed once: a B-view gradient is the sum of the per-view references; padded-M, packed and fused variants reuse them."""
import collections
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import aa_reference
import oracle
from helpers import cov3d_from, make_scene
from humangaussian_amd import synth
from oracle import OracleSettings

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
H, W = 48, 64
GRAD_TOL, COS_TOL = 1e-3, 1e-5
MAX_VIEWS = 16
ACT_ALL = 1 | 2 | 4            # ACT_OPACITY_SIGMOID | ACT_SCALE_EXP | ACT_ROTATION_NORMALIZE (humangaussian_amd/rasterizer.py)

# ------------------------------------------------------------------------------------------------- the case table
# B views, SH degree, filter, stored SH coefficients M (0: colors_precomp), P Gaussians, colour input ("sh" / "precomp":
# the settings then say sh_degree 3 and the degree-0 kernel must still serve), covariance input ("sr": scales + rotations /
# "cov": cov3D_precomp), scale_modifier, output ("six" tensors / the "packed" row), fused activations
Case = collections.namedtuple("Case", "B deg aa M P color cov mod out fused")


def _c(B, deg, aa, M, P, color="sh", cov="sr", mod=1.0, out="six", fused=False):
    return Case(B, deg, bool(aa), M if color == "sh" else 0, P, color, cov, mod, out, fused)


def case_id(c):
    return (f"B{c.B}-deg{c.deg}-{'aa' if c.aa else 'off'}-M{c.M}-P{c.P}-{c.color}-{c.cov}-mod{c.mod}-{c.out}"
            + ("-fused" if c.fused else ""))


def _one_view(aa):
    return [
        # degree 0 (never staged): scalar M == NC, vector M > NC, packed; precomputed colours under sh_degree 3
        _c(1, 0, aa, 1, 1), _c(1, 0, aa, 1, 577), _c(1, 0, aa, 16, 256), _c(1, 0, aa, 1, 63, out="packed"),
        _c(1, 0, aa, 16, 257, out="packed"), _c(1, 0, aa, 0, 255, color="precomp", cov="cov"),
        _c(1, 0, aa, 0, 577, color="precomp", mod=0.7), _c(1, 0, aa, 16, 577, fused=True),
        # degree 1: staged (P >= 256, 4 <= M <= 16) / vector (M = 4, 16) / scalar (M = 5, 10, 25); 577 = two staged chunks + a tail
        _c(1, 1, aa, 4, 577), _c(1, 1, aa, 4, 255), _c(1, 1, aa, 5, 577), _c(1, 1, aa, 10, 256), _c(1, 1, aa, 16, 257),
        _c(1, 1, aa, 25, 577), _c(1, 1, aa, 16, 63), _c(1, 1, aa, 5, 1), _c(1, 1, aa, 4, 256, out="packed"),
        _c(1, 1, aa, 10, 577, out="packed"), _c(1, 1, aa, 5, 577, cov="cov"), _c(1, 1, aa, 10, 577, mod=0.7, fused=True),
        # degree 2: staged M = 9, 10, 13, 16; scalar M = 9 (==), 10, 13; vector M = 16
        _c(1, 2, aa, 9, 577), _c(1, 2, aa, 9, 63), _c(1, 2, aa, 10, 257), _c(1, 2, aa, 13, 577), _c(1, 2, aa, 16, 256),
        _c(1, 2, aa, 16, 255), _c(1, 2, aa, 13, 255), _c(1, 2, aa, 9, 577, out="packed"),
        _c(1, 2, aa, 16, 257, out="packed", fused=True), _c(1, 2, aa, 9, 257, mod=0.7),
        # degree 3: staged / vector M = 16 (==), scalar M = 25 (neither staged nor vectorised)
        _c(1, 3, aa, 16, 577), _c(1, 3, aa, 16, 255), _c(1, 3, aa, 16, 256), _c(1, 3, aa, 25, 577), _c(1, 3, aa, 25, 257),
        _c(1, 3, aa, 16, 577, out="packed"), _c(1, 3, aa, 25, 63, out="packed"), _c(1, 3, aa, 16, 577, cov="cov"),
        _c(1, 3, aa, 16, 257, fused=True),
    ]


def _many_views(aa):
    return [
        # thread per (Gaussian, view): 2..16 views at degrees 0 / 1 (16: the raised LDS limit), 2..8 at degrees 2 / 3;
        # groups of 64 Gaussians: P = 63, 64, 65 on purpose
        _c(2, 0, aa, 1, 63), _c(16, 0, aa, 16, 577), _c(3, 0, aa, 1, 64, out="packed"), _c(8, 0, aa, 16, 577, out="packed"),
        _c(2, 0, aa, 0, 577, color="precomp", cov="cov"),
        _c(2, 1, aa, 4, 65), _c(16, 1, aa, 5, 577), _c(8, 1, aa, 16, 577), _c(3, 1, aa, 25, 64), _c(3, 1, aa, 10, 577, fused=True),
        _c(2, 1, aa, 4, 577, out="packed"), _c(16, 1, aa, 10, 577, out="packed"), _c(3, 1, aa, 4, 577, mod=0.7),
        _c(8, 2, aa, 9, 577), _c(2, 2, aa, 10, 63), _c(3, 2, aa, 16, 65), _c(3, 2, aa, 13, 577), _c(2, 2, aa, 9, 577, cov="cov"),
        _c(8, 2, aa, 9, 577, out="packed"), _c(2, 2, aa, 13, 64, out="packed"), _c(3, 2, aa, 16, 577, out="packed"),
        _c(8, 3, aa, 16, 577), _c(2, 3, aa, 25, 65), _c(3, 3, aa, 16, 64), _c(3, 3, aa, 16, 577, out="packed"),
        _c(8, 3, aa, 25, 577, out="packed", fused=True),
        # the loop over the views: 9..16 views at degrees 2 / 3 (9: the form switch)
        _c(9, 2, aa, 9, 577), _c(16, 2, aa, 10, 577), _c(9, 2, aa, 16, 65), _c(9, 2, aa, 13, 577, fused=True),
        _c(9, 2, aa, 9, 64, out="packed"), _c(16, 2, aa, 16, 577, out="packed"),
        _c(9, 3, aa, 16, 577), _c(16, 3, aa, 25, 577), _c(9, 3, aa, 16, 63), _c(16, 3, aa, 16, 577, out="packed"),
        _c(9, 3, aa, 25, 65, out="packed"),
    ]


CASES = _one_view(False) + _one_view(True) + _many_views(False) + _many_views(True)
MULTI_VIEW_CASES = [c for c in CASES if c.B > 1]
# the handful that also goes through the raw C ABI (tests/abi_runner.py: every output NaN-filled by the caller)
RAW_ABI_CASES = [c for c in CASES if c.B == 1 and not c.aa and c.out == "six" and not c.fused and c.cov == "sr" and c.mod == 1.0
                 and (c.deg, c.M, c.P) in {(0, 16, 256), (1, 5, 577), (1, 25, 577), (2, 13, 577), (3, 16, 577), (3, 25, 257)}]


# ------------------------------------------------------------------------------------------------- scenes and references
def nc_of(deg):
    return (deg + 1) ** 2


_CAMS, _SCENES, _REFS = [], {}, {}
# The scenes' seeds start here.  Not every seed serves: where the oracle's own fp32 run takes a hard decision of the blend
# (alpha >= 1/255) differently from its fp64 run, any fp32 implementation is a finite step away from fp64 on that Gaussian
# (tests/helpers.py: "flip Gaussians").  tests/test_pre_bwd_matrix_cpu.py checks every (scene, view) of the table for it, on
# the reference alone.
SEED_BASE = 27000


def cameras():
    """the 16 cameras every case takes its first B views from"""
    if not _CAMS:
        g = torch.Generator().manual_seed(2718)
        for i in range(MAX_VIEWS):
            r = torch.rand(4, generator=g).tolist()
            _CAMS.append(synth.orbit_camera(-30 + 60 * r[0], -180 + 360 * (i + r[1]) / MAX_VIEWS, 1.7 + 0.6 * r[2],
                                            45 + 20 * r[3], H, W))
    return _CAMS


def scene(deg, P):
    """One cloud per (degree, P), whatever M, the inputs' kind and the number of views: 25 stored SH coefficients (a case
    takes the first M; the inactive ones are random and non-zero); from 32 Gaussians on three of them sit behind cameras
    0, 1, 2 (culled there: rows without entries are written too)."""
    if (deg, P) not in _SCENES:
        sc = make_scene(P=P, sh_degree=deg, M=25, seed=SEED_BASE + 10 * P + deg, H=H, W=W, spread=0.3, scale=0.02)
        if P >= 32:
            for j, idx in enumerate((0, P // 2, P - 1)):
                sc["means3D"][idx] = 2.0 * torch.as_tensor(cameras()[j].camera_center, dtype=torch.float32)
        g = torch.Generator().manual_seed(9000 + 10 * P + deg)
        sc["colors_precomp"] = torch.rand(P, 3, generator=g)
        sc["rot_stretch"] = 0.5 + torch.rand(P, 1, generator=g)        # fused cases: |raw quaternion| in 0.5 .. 1.5
        assert float(sc["shs"][:, 1:].abs().min()) > 0
        _SCENES[(deg, P)] = sc
    return _SCENES[(deg, P)]


def upstream(view):
    """seeded N(0, 1) incoming gradients on the three heads of view `view`"""
    g = torch.Generator().manual_seed(1000 + view)
    return [torch.randn(s, generator=g) for s in ((3, H, W), (1, H, W), (1, H, W))]


def activated_inputs(c):
    """what the oracle gets (CPU, fp32): the scene's ACTIVATED parameters, SH cut to the active coefficients"""
    sc = scene(c.deg, c.P)
    ins = {"means3D": sc["means3D"], "opacities": sc["opacities"]}
    if c.color == "sh":
        ins["shs"] = sc["shs"][:, :nc_of(c.deg)].contiguous()
    else:
        ins["colors_precomp"] = sc["colors_precomp"]
    if c.cov == "sr":
        ins["scales"], ins["rotations"] = sc["scales"], sc["rotations"]
    else:
        ins["cov3D_precomp"] = cov3d_from(sc)
    return ins


def ref_key(c, view):
    return (c.deg, c.P, c.aa, c.color, c.cov, c.mod, view)


def _oracle_settings(c, view):
    cam, sc = cameras()[view], scene(c.deg, c.P)
    return OracleSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), sc["bg"], c.mod,
                          cam.world_view_transform, cam.full_proj_transform, c.deg if c.color == "sh" else 3,
                          cam.camera_center, False, False)


def reference_view(c, view, dtype=torch.float64):
    """the oracle's gradients (and radii) of one view of the case's scene; cached across the cases that share it"""
    key = ref_key(c, view) + (dtype,)
    if key not in _REFS:
        ins = activated_inputs(c)
        fb = aa_reference.forward_backward if c.aa else oracle.forward_backward
        with torch.enable_grad():
            out = fb(ins["means3D"], ins.get("shs"), ins.get("colors_precomp"), ins["opacities"], ins.get("scales"),
                     ins.get("rotations"), ins.get("cov3D_precomp"), _oracle_settings(c, view), *upstream(view), dtype=dtype)
        _REFS[key] = ({k: v.detach().double() for k, v in out["grads"].items()}, out["radii"])
    return _REFS[key]


def reference(c, dtype=torch.float64):
    """the B-view reference: parameter gradients summed over the views, means2D per view (B, P, 3); visible (P,)"""
    per = [reference_view(c, b, dtype) for b in range(c.B)]
    g = {k: sum(p[0][k] for p in per) for k in per[0][0] if k != "means2D"}
    g["means2D"] = torch.stack([p[0]["means2D"] for p in per])
    if c.fused:
        g.update(_chain_activations(raw_inputs(c), g))
    visible = torch.stack([p[1] > 0 for p in per]).any(0)
    return g, visible


def _chain_activations(raw, g):
    """fp64 autograd of sigmoid / exp / normalize at the raw inputs, applied to the gradients w.r.t. the activated ones"""
    leaves = {k: raw[k].double().requires_grad_(True) for k in ("opacities", "scales", "rotations")}
    with torch.enable_grad():
        acts = [torch.sigmoid(leaves["opacities"]), torch.exp(leaves["scales"]),
                torch.nn.functional.normalize(leaves["rotations"], dim=1)]
        gl = torch.autograd.grad(acts, list(leaves.values()), [g[k].reshape(leaves[k].shape) for k in leaves])
    return dict(zip(leaves, gl))


def raw_inputs(c):
    """what the rasterizer gets (CPU, fp32): M stored coefficients; fused: the model's raw parameters.  (sigmoid(logit(p)) and
    exp(log(s)) return p and s to an fp32 rounding, 1e-7 relative: the reference at the scene's own values serves both.)"""
    sc, ins = scene(c.deg, c.P), dict(activated_inputs(c))
    if c.color == "sh":
        ins["shs"] = sc["shs"][:, :c.M].contiguous()
    if c.fused:
        ins["opacities"] = torch.logit(sc["opacities"])
        ins["scales"] = torch.log(sc["scales"])
        ins["rotations"] = sc["rotations"] * sc["rot_stretch"]
    return ins


# ------------------------------------------------------------------------------------------------- the device side
def _settings(c, view):
    from humangaussian_amd import GaussianRasterizationSettings
    cam, sc = cameras()[view], scene(c.deg, c.P)
    return GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), sc["bg"].to(DEV), c.mod,
                                         cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV),
                                         c.deg if c.color == "sh" else 3, cam.camera_center.to(DEV), False, False)


def _poison(B, P, M):
    """Fill the blocks the caching allocator will hand to the next `at::empty` of a gradient's size with NaN: an element
    the backward does not write is then NaN, not a lucky zero."""
    shapes = [(P, 3), (B, P, 3), (P, max(M, 1), 3), (P, 1), (P, 4), (P, 6), (P, 15 + 3 * max(M, 1))]
    junk = [torch.full(s, float("nan"), device=DEV) for s in shapes for _ in range(3)]
    del junk
    for s in shapes:
        torch.empty(s, device=DEV).fill_(float("nan"))


def run_views(c, views, packed=False, raw=None):
    """forward + backward of the case's inputs under the given views; -> dict(color, depth, alpha, radii, grads, pack) on the CPU.
    One view without fused activations: through GaussianRasterizer; else through rasterize_gaussians_batch."""
    from humangaussian_amd import GaussianRasterizer, rasterize_gaussians_batch
    from humangaussian_amd import rasterizer as R
    raw = raw_inputs(c) if raw is None else raw
    ins = {k: v.to(DEV).requires_grad_(True) for k, v in raw.items()}
    B, P, M = len(views), c.P, int(raw["shs"].shape[1]) if "shs" in raw else 0
    rsl = [_settings(c, v) for v in views]
    ups = [upstream(v) for v in views]
    _poison(B, P, M)
    if B == 1 and not c.fused:
        m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
        outs = GaussianRasterizer(rsl[0], antialiasing=c.aa)(
            means3D=ins["means3D"], means2D=m2, opacities=ins["opacities"], shs=ins.get("shs"),
            colors_precomp=ins.get("colors_precomp"), scales=ins.get("scales"), rotations=ins.get("rotations"),
            cov3D_precomp=ins.get("cov3D_precomp"))
        gouts = [t.to(DEV) for t in ups[0]]
    else:
        m2 = torch.zeros(B, P, 3, device=DEV, requires_grad=True)
        outs = rasterize_gaussians_batch(ins["means3D"], m2, ins.get("shs"), ins.get("colors_precomp"), ins["opacities"],
                                         ins.get("scales"), ins.get("rotations"), ins.get("cov3D_precomp"), rsl,
                                         activation_flags=ACT_ALL if c.fused else 0, antialiasing=c.aa)
        gouts = [torch.stack([u[i] for u in ups]).to(DEV) for i in range(3)]
    color, radii, depth, alpha = outs
    names = list(ins) + ["means2D"]
    tens = list(ins.values()) + [m2]
    _poison(B, P, M)
    pack = None
    if packed:
        with R.packed_gradients() as pg:
            gl = torch.autograd.grad([color, depth, alpha], tens, gouts)
            pack = pg.take()
        assert pack is not None, "the packed backward did not run"
    else:
        gl = torch.autograd.grad([color, depth, alpha], tens, gouts)
    torch.cuda.synchronize()
    return dict(color=color.detach().cpu(), depth=depth.detach().cpu(), alpha=alpha.detach().cpu(), radii=radii.cpu(),
                grads={k: g.detach().cpu().reshape((B, P, 3) if k == "means2D" else g.shape) for k, g in zip(names, gl)},
                pack=None if pack is None else pack.cpu())


def run_case(c, packed=None):
    return run_views(c, list(range(c.B)), packed=(c.out == "packed") if packed is None else packed)


def gate(got, ref, what):
    """finite; within GRAD_TOL of max|g64|; cosine >= 1 - COS_TOL"""
    assert torch.isfinite(got).all(), (what, "non-finite", int((~torch.isfinite(got)).sum()))
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    scale = max(float(ref.abs().max()), 1e-12)
    err = float((got - ref).abs().max()) / scale
    cos = float(torch.dot(got, ref) / (got.norm() * ref.norm())) if float(ref.norm()) > 0 else 1.0
    print(f"{what}: err {err:.2e} of max|g64|, 1 - cos {1 - cos:.1e}")
    assert err <= GRAD_TOL, (what, err)
    assert cos >= 1 - COS_TOL, (what, cos)


def gate_all(c, grads, ref, what):
    assert set(grads) == set(ref), (set(grads), set(ref))
    for k in ref:
        got = grads[k]
        if k == "shs":
            nc = nc_of(c.deg)
            rest = got[:, nc:].contiguous()
            assert bool((rest.view(torch.int32) == 0).all()), (what, "the gradient of the inactive SH coefficients is not bitwise zero",
                                                               int((rest.view(torch.int32) != 0).sum()))
            got = got[:, :nc]
        gate(got, ref[k], (what, k))


def bitwise(a, b):
    """torch.equal: no tolerance; a NaN equals nothing (a sum that starts at +0 turns a -0 term into +0: the signs of zeros
    are not compared)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def view_ordered_sum(x):
    acc = x[0].clone()
    for b in range(1, x.shape[0]):
        acc += x[b]
    return acc


# ------------------------------------------------------------------------------------------------- the second build
def _max_views_of_the_header():
    with open(os.path.join(ROOT, "include", "hgs_rast.h")) as f:
        return int(re.search(r"#define\s+HGS_MAX_VIEWS\s+(\d+)", f.read()).group(1))


class _DlInfo(ctypes.Structure):
    _fields_ = [("dli_fname", ctypes.c_char_p), ("dli_fbase", ctypes.c_void_p), ("dli_sname", ctypes.c_char_p),
                ("dli_saddr", ctypes.c_void_p)]


def _library_serving(symbol="hgs_backward_batch_act"):
    """the shared object the process resolves `symbol` to (what the torch binding's calls reach)"""
    glob = ctypes.CDLL(None)
    info = _DlInfo()
    glob.dladdr.argtypes = [ctypes.c_void_p, ctypes.POINTER(_DlInfo)]
    assert glob.dladdr(ctypes.cast(getattr(glob, symbol), ctypes.c_void_p), ctypes.byref(info)) != 0
    return os.path.realpath(info.dli_fname.decode())


def _loop_form_worker(out_path):
    """(the child process, running on the second build) every multi-view case of the table"""
    from humangaussian_amd import _lib
    _lib.load_binding()
    assert _library_serving() == os.path.realpath(os.environ["HGS_LIB"]), (_library_serving(), os.environ["HGS_LIB"])
    res = {}
    for c in MULTI_VIEW_CASES:
        r = run_case(c)
        res[case_id(c)] = dict(grads=r["grads"], pack=r["pack"], radii=r["radii"])
    torch.save(res, out_path)


@pytest.fixture(scope="module", autouse=True)
def loop_form(tmp_path_factory):
    """What `_loop_form_worker` produced on a second build of the same sources with HGS_PRE_BWD_VPAR_MIN_VIEWS above
    HGS_MAX_VIEWS (same flags otherwise; never installed): every multi-view backward takes the loop form there.  One child
    process for the whole table, under its own time limit.  Every test of the module depends on it: if the child ends
    abnormally, nothing else of the module runs on the GPU."""
    tmp = tmp_path_factory.mktemp("loopform")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the loop-form comparison build needs hipcc on the GPU box"
    csrc = os.path.join(ROOT, "humangaussian_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
             f"-DHGS_PRE_BWD_VPAR_MIN_VIEWS={_max_views_of_the_header() + 1}"]
    procs = [subprocess.Popen([hipcc] + flags + ["-c", os.path.join(csrc, src), "-o", str(tmp / (src + ".o"))])
             for src in ("api.hip", "render_bwd.hip")]
    assert all(p.wait() == 0 for p in procs)
    twin = str(tmp / "libhgs_rast.so")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", str(tmp / "api.hip.o"),
                           str(tmp / "render_bwd.hip.o"), "-o", twin])
    # the torch binding is linked against the in-tree library: the second build has to come first in the lookup order
    # (appended to whatever is preloaded already)
    preload = os.pathsep.join(x for x in (os.environ.get("LD_PRELOAD", ""), twin) if x)
    env = dict(os.environ, LD_PRELOAD=preload, HGS_LIB=twin,
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [x for x in (os.environ.get("PYTHONPATH"),) if x]))
    code = "import test_gpu_pre_bwd_matrix as T; T._loop_form_worker(%r)" % str(tmp / "loop.pt")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return torch.load(tmp / "loop.pt")


# ------------------------------------------------------------------------------------------------- 1. the table against fp64
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_against_the_fp64_oracle(c):
    ref, visible = reference(c)
    r = run_case(c)
    gate_all(c, r["grads"], ref, case_id(c))
    culled = ~visible
    if bool(culled.any()):                       # a Gaussian no view sees: every row exactly zero
        for k, g in r["grads"].items():
            rows = g[:, culled] if k == "means2D" else g[culled]
            assert float(rows.abs().max()) == 0.0, (case_id(c), k)
    if c.out == "packed":
        from humangaussian_amd import view_parallel as vp
        u = run_case(c, packed=False)
        for k in u["grads"]:
            assert bitwise(u["grads"][k], r["grads"][k]), (case_id(c), k, "packed views differ from the six tensors")
        radii = u["radii"].reshape(c.B, c.P).max(dim=0).values.to(torch.int32)
        want = vp.pack_contribution({**u["grads"], "means2D": view_ordered_sum(u["grads"]["means2D"])}, radii)
        assert bitwise(r["pack"], want), (case_id(c), float((r["pack"] - want).abs().max()))


@pytest.mark.parametrize("c", RAW_ABI_CASES, ids=case_id)
def test_case_through_the_raw_abi(c):
    from abi_runner import RawCall
    assert len(RAW_ABI_CASES) == 6
    sc, raw = scene(c.deg, c.P), raw_inputs(c)
    rc = RawCall(dict(sc, shs=raw["shs"], cam=cameras()[0]), scale_modifier=c.mod, sh_degree=c.deg)
    assert rc.forward() == 0 and not rc.status[4]
    got = rc.backward(*upstream(0))
    ref, _ = reference(c)
    gate_all(c, {k: (v.reshape(1, c.P, 3) if k == "means2D" else v) for k, v in got.items() if v is not None}, ref,
             "raw ABI " + case_id(c))


# ------------------------------------------------------------------------------------------------- 2. bit-for-bit relations
PAD_M = {0: (1, 16, 5, 25), 1: (4, 16, 5, 10, 25), 2: (9, 16, 10, 13, 25), 3: (16, 17, 25)}


@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("aa", [False, True], ids=["off", "aa"])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_padding_the_sh_storage_changes_no_bit(deg, aa, B):
    """M = NC, 16, odd layouts, 25 on the same scene: images and every gradient identical on the shared part - the staged,
    vector and scalar SH paths (and the packed row) against each other."""
    nc = nc_of(deg)
    base = None
    for out in ("six", "packed"):
        for M in PAD_M[deg]:
            c = _c(B, deg, aa, M, 577, out=out)
            r = run_case(c)
            sh = r["grads"].pop("shs")
            assert bool((sh[:, nc:].contiguous().view(torch.int32) == 0).all()), (out, M)
            r["grads"]["shs_active"] = sh[:, :nc].contiguous()
            if base is None:
                base = r
                continue
            for k in ("color", "depth", "alpha", "radii"):
                assert bitwise(r[k], base[k]), (out, M, k)
            for k in base["grads"]:
                assert bitwise(r["grads"][k], base["grads"][k]), (out, M, k, float((r["grads"][k] - base["grads"][k]).abs().max()))


@pytest.mark.parametrize("B,deg", [(9, 2), (16, 2), (9, 3), (16, 3), (16, 0), (16, 1)])
def test_batched_call_equals_the_per_view_calls_summed_in_view_order(B, deg):
    """without the filter: `d2` / `d3` with the run-time bit off (9, 16 views), the raised LDS limit (16 views, degrees 0, 1)"""
    c = _c(B, deg, False, nc_of(deg), 577)
    r = run_case(c)
    singles = [run_views(c, [b]) for b in range(B)]
    for b, s in enumerate(singles):
        for k in ("color", "depth", "alpha"):
            assert bitwise(r[k][b], s[k]), (b, k)
        assert bitwise(r["radii"][b], s["radii"]), b
        assert bitwise(r["grads"]["means2D"][b], s["grads"]["means2D"][0]), b
    for k in r["grads"]:
        if k != "means2D":
            want = view_ordered_sum(torch.stack([s["grads"][k] for s in singles]))
            assert bitwise(r["grads"][k], want), (k, float((r["grads"][k] - want).abs().max()))


@pytest.mark.parametrize("c", MULTI_VIEW_CASES, ids=case_id)
def test_loop_form_equals_the_default_form_bitwise(c, loop_form):
    """preprocess.hip, mode 2: "the same sequence of fp32 additions as the loop of mode 0" - every multi-view case of the
    table in the build that always loops (`d0` .. `d3`, `d0_aa` .. `d2_aa`) and in the shipped one."""
    a, b = run_case(c), loop_form[case_id(c)]
    assert bitwise(a["radii"], b["radii"])
    for k in a["grads"]:
        assert bitwise(a["grads"][k], b["grads"][k]), (k, float((a["grads"][k] - b["grads"][k]).abs().max()))
    if c.out == "packed":
        assert bitwise(a["pack"], b["pack"])


# ------------------------------------------------------------------------------------------------- 3. fused activations at the edges
EDGE_P, EDGE_DEG, EDGE_M = 577, 2, 10
EDGE_OPACITY = (12.0, -12.0, 30.0, -30.0)
_EDGE = {}


def edge_raw():
    """Raw parameters at the edges of what a model holds, all finite: opacity logits including +-12 and +-30 (sigmoid
    saturates: 1 - 6e-6, 6e-6, 1 in fp32, 9e-14), quaternions scaled per row by 1e-3 .. 1e3, log-scales from -9 to 0
    (most rows keep the scene's own, around -4; rows 100.. are set to the ends and in between)."""
    if not _EDGE:
        sc = scene(EDGE_DEG, EDGE_P)
        g = torch.Generator().manual_seed(31415)
        op = torch.logit(sc["opacities"]).clone()
        for j, v in enumerate(EDGE_OPACITY * 6):
            op[10 + 3 * j] = v
        stretch = 10.0 ** (6.0 * torch.rand(EDGE_P, 1, generator=g) - 3.0)
        stretch[20], stretch[21], stretch[22] = 1e-3, 1e3, 1.0
        ls = torch.log(sc["scales"]).clone().clamp(-9.0, 0.0)
        ls[100:108] = -9.0
        ls[108:116, 0] = -9.0
        ls[116:120] = 0.0
        ls[120:124, 1] = 0.0
        ls[124:140] = torch.linspace(-8.0, -1.0, 16)[:, None]
        _EDGE.update(means3D=sc["means3D"], shs=sc["shs"][:, :EDGE_M].contiguous(), opacities=op, scales=ls,
                     rotations=sc["rotations"] * stretch)
        assert all(bool(torch.isfinite(v).all()) for v in _EDGE.values())
    return _EDGE


def edge_reference(B, aa, dtype=torch.float64):
    """fp64 autograd of sigmoid / exp / normalize composed with the oracle, at the raw inputs"""
    raw = edge_raw()
    c = _c(1, EDGE_DEG, aa, EDGE_M, EDGE_P)
    per = []
    for b in range(B):
        key = ("edge", aa, dtype, b)
        if key not in _REFS:
            d = {k: v.to(dtype) for k, v in raw.items()}
            fb = aa_reference.forward_backward if aa else oracle.forward_backward
            with torch.enable_grad():
                out = fb(d["means3D"], d["shs"][:, :nc_of(EDGE_DEG)].contiguous(), None, torch.sigmoid(d["opacities"]),
                         torch.exp(d["scales"]), torch.nn.functional.normalize(d["rotations"], dim=1), None,
                         _oracle_settings(c, b), *upstream(b), dtype=dtype)
            _REFS[key] = {k: v.detach().double() for k, v in out["grads"].items()}
        per.append(_REFS[key])
    g = {k: sum(p[k] for p in per) for k in per[0] if k != "means2D"}
    g["means2D"] = torch.stack([p["means2D"] for p in per])
    g.update(_chain_activations(raw, g))
    return g


def rows_without_reference_gradient(ref, P):
    dead = torch.ones(P, dtype=torch.bool)
    for k, g in ref.items():
        per_row = g.reshape(-1, P, g.shape[-1]).abs().amax(dim=(0, 2)) if k == "means2D" else g.reshape(P, -1).abs().amax(dim=1)
        dead &= per_row == 0
    return dead


@pytest.mark.parametrize("out", ["six", "packed"])
@pytest.mark.parametrize("aa", [False, True], ids=["off", "aa"])
@pytest.mark.parametrize("B", [1, 3])
def test_fused_activations_at_the_edges(B, aa, out):
    c = _c(B, EDGE_DEG, aa, EDGE_M, EDGE_P, out=out, fused=True)
    ref = edge_reference(B, aa)
    r = run_views(c, list(range(B)), packed=out == "packed", raw=edge_raw())
    gate_all(c, r["grads"], ref, f"edges B{B} {'aa' if aa else 'off'} {out}")
    # a Gaussian the reference gives no gradient at all (below the 1/255 threshold everywhere: the saturated logits; culled): exactly 0
    dead = rows_without_reference_gradient(ref, EDGE_P)
    assert int(dead.sum()) >= 12, int(dead.sum())                    # (the twelve rows at -12 and -30)
    for k, g in r["grads"].items():
        rows = g[:, dead] if k == "means2D" else g[dead]
        assert float(rows.abs().max()) == 0.0, (k, "a row with no reference gradient is not exactly zero")
