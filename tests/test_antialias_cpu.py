"""CPU side of the opt-in antialiasing filter (HGS_ANTIALIAS, ABI v17): the fp64 reference (tests/aa_reference.py) is a
differentiable function with the clamp where upstream has it, the C ABI accepts the bit, and every layer of the Python
API hands it to the binding (a recording stand-in for _lib.load_binding(): no GPU here)."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

import aa_reference
from helpers import make_scene
from humangaussian_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib, rasterize_gaussians_batch, synth
from humangaussian_amd import rasterizer as R
from humangaussian_amd import renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the fp64 reference
def test_rho_gradcheck_including_the_clamp():
    h = 0.3
    # (a0, b, c0) before the dilation: large, small, elongated, and one held at the clamp (det0 < 0 -> ratio < 2.5e-5)
    a0 = torch.tensor([4.0, 0.05, 2.0, 1e-4], dtype=torch.float64)
    b = torch.tensor([0.5, 0.01, 1.9, 0.2], dtype=torch.float64)
    c0 = torch.tensor([3.0, 0.04, 1.9, 1e-4], dtype=torch.float64)
    cov = torch.stack([a0 + h, b, c0 + h], 1).requires_grad_(True)
    det0, det = a0 * c0 - b * b, (a0 + h) * (c0 + h) - b * b
    assert float(det0[3] / det[3]) < aa_reference.MIN_RATIO
    rho = aa_reference.rho_of(cov).detach()
    assert float(rho[3]) == pytest.approx(math.sqrt(aa_reference.MIN_RATIO))
    assert torch.allclose(rho[:3], torch.sqrt(det0[:3] / det[:3]))
    assert torch.autograd.gradcheck(aa_reference.rho_of, (cov,))
    g, = torch.autograd.grad(aa_reference.rho_of(cov)[3], cov)
    assert float(g.abs().max()) == 0.0                      # under the clamp rho is a constant
    # the chain rule the kernels use (include/hgs_rast.h): d rho / d(a, b, c) with rho^2 = det0 / det
    g, = torch.autograd.grad(aa_reference.rho_of(cov)[:3].sum(), cov)
    r2 = det0[:3] / det[:3]
    k = 1.0 / (2.0 * torch.sqrt(r2) * det[:3])
    a, c = a0[:3] + h, c0[:3] + h
    assert torch.allclose(g[:3, 0], k * (c0[:3] - r2 * c))
    assert torch.allclose(g[:3, 2], k * (a0[:3] - r2 * a))
    assert torch.allclose(g[:3, 1], -2.0 * k * b[:3] * (1.0 - r2))


def test_rho_tends_to_one_for_large_gaussians():
    a0 = torch.tensor([1e2, 1e4, 1e6], dtype=torch.float64)
    cov = torch.stack([a0 + 0.3, torch.zeros(3, dtype=torch.float64), a0 + 0.3], 1)
    rho = aa_reference.rho_of(cov)
    assert bool((rho < 1).all()) and float(1 - rho[-1]) < 1e-6 and float(1 - rho[0]) < 1e-2


def test_reference_rasterize_gradcheck_small_scene():
    sc = make_scene(P=6, sh_degree=1, seed=3, H=16, W=16, spread=0.15, scale=0.01)
    from helpers import oracle_settings
    st = oracle_settings(sc)
    sh = sc["shs"].double()
    w = torch.Generator().manual_seed(1)
    wa = torch.randn(1, 16, 16, generator=w, dtype=torch.float64)

    def f(means, opac, scales):
        _, _, _, alpha = aa_reference.rasterize(means, None, sh, None, opac, scales, sc["rotations"].double(), None, st,
                                                dtype=torch.float64)
        return (alpha * wa).sum()
    ins = tuple(sc[k].double().requires_grad_(True) for k in ("means3D", "opacities", "scales"))
    with aa_reference.antialiased():
        from oracle import gs_oracle
        pre = gs_oracle.preprocess(*(t.detach() for t in ins[:1]), None, sh, None, ins[1].detach(), ins[2].detach(),
                                   sc["rotations"].double(), None, st, dtype=torch.float64)
    assert bool((pre["rho"][pre["visible"]] < 0.9).any())      # the filter bites in this scene
    assert torch.autograd.gradcheck(f, ins, eps=1e-7, atol=1e-5, rtol=1e-3)


def test_committed_filter_ratio_matches_fp64_reference():
    import test_gpu_antialias
    ratio, errs = aa_reference.filter_error_ratio_fp64()
    assert errs[False] > 0 and ratio < 0.5
    assert ratio == pytest.approx(test_gpu_antialias.FILTER_RATIO_FP64, rel=1e-3)


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_and_lib_agree_on_the_bit_and_the_abi():
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    assert re.search(r"^#define HGS_ANTIALIAS 16\b", hdr, flags=re.M)
    assert R.ANTIALIAS == 16 and _lib.ABI_VERSION == 17
    _lib.build()
    assert _lib.load().hgs_abi_version() == 17


def _settings_struct():
    keep = [torch.zeros(16) for _ in range(4)]
    s = _lib.HgsSettings()
    s.image_height, s.image_width, s.tanfovx, s.tanfovy = 16, 16, 0.5, 0.5
    s.bg, s.viewmatrix, s.projmatrix, s.campos = (t.data_ptr() for t in keep)
    s.scale_modifier, s.sh_degree = 1.0, 0
    return s, keep


def test_backward_accepts_the_bit_and_rejects_unknown_bits():
    lib = _lib.load()
    s, keep = _settings_struct()
    dummy = torch.zeros(64, dtype=torch.uint8)
    p = ctypes.c_void_p(dummy.data_ptr())

    def bwd(flags):          # P = 0: argument checks only, nothing reaches a device
        return lib.hgs_backward_batch_act(ctypes.byref(s), 1, 0, 1, *([None] * 8), *([None] * 6), p, p, p, None, 0, None,
                                          *([None] * 8), None, flags, None)
    assert bwd(0) == 0
    assert bwd(R.ANTIALIAS) == 0
    assert bwd(R.ANTIALIAS | R.ACT_OPACITY_SIGMOID | R.ACT_SCALE_EXP | R.ACT_ROTATION_NORMALIZE | R.GRAD_SCALE_TRUE_DERIVATIVE) == 0
    assert bwd(32) == -1 and bwd(R.ANTIALIAS | 32) == -1
    del keep


# ------------------------------------------------------------------------------------------------------- the plumbing
class _Recorder:
    """Stands in for the torch binding: records the flags of every rasterize call, returns zero outputs."""

    def __init__(self):
        self.calls = []

    def rasterize(self, means3D, *args):
        self.calls.append(("single", int(args[-1])))
        H, W = int(args[11]), int(args[12])
        P = means3D.shape[0]
        return torch.zeros(3, H, W), torch.zeros(P, dtype=torch.int32), torch.zeros(1, H, W), torch.zeros(1, H, W)

    def rasterize_batch(self, means3D, *args):
        self.calls.append(("batch", int(args[-1])))
        B, H, W, P = len(args[13]), int(args[11]), int(args[12]), means3D.shape[0]
        return (torch.zeros(B, 3, H, W), torch.zeros(B, P, dtype=torch.int32), torch.zeros(B, 1, H, W),
                torch.zeros(B, 1, H, W))


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(_lib, "load_binding", lambda: r)
    return r


def _scene_and_settings(deg=0):
    sc = make_scene(P=10, sh_degree=deg, seed=0, H=32, W=32)
    cam = sc["cam"]
    rs = GaussianRasterizationSettings(cam.image_height, cam.image_width, math.tan(cam.FoVx * 0.5),
                                       math.tan(cam.FoVy * 0.5), sc["bg"], 1.0, cam.world_view_transform,
                                       cam.full_proj_transform, deg, cam.camera_center, False, False)
    return sc, rs


def _call(rast, sc):
    return rast(means3D=sc["means3D"], means2D=torch.zeros_like(sc["means3D"]), shs=sc["shs"], opacities=sc["opacities"],
                scales=sc["scales"], rotations=sc["rotations"])


def _aa(flags):
    return bool(flags & R.ANTIALIAS)


def test_rasterizer_sends_the_bit(rec):
    sc, rs = _scene_and_settings()
    _call(GaussianRasterizer(rs), sc)
    _call(GaussianRasterizer(rs, antialiasing=False), sc)
    _call(GaussianRasterizer(rs, antialiasing=True), sc)
    assert [_aa(f) for _, f in rec.calls] == [False, False, True]
    # a settings object in the style of upstream's 13-field settings (`antialiasing` after `debug`)
    rs13 = types.SimpleNamespace(**rs._asdict(), antialiasing=True)
    _call(GaussianRasterizer(rs13), sc)
    assert _aa(rec.calls[-1][1])
    _call(GaussianRasterizer(rs13, antialiasing=False), sc)          # an explicit choice overrides the settings
    assert not _aa(rec.calls[-1][1])
    R.rasterize_gaussians(sc["means3D"], torch.zeros_like(sc["means3D"]), sc["shs"], None, sc["opacities"], sc["scales"],
                          sc["rotations"], None, rs13, antialiasing=False)
    assert rec.calls[-1] == ("single", 0)
    R.rasterize_gaussians(sc["means3D"], torch.zeros_like(sc["means3D"]), sc["shs"], None, sc["opacities"], sc["scales"],
                          sc["rotations"], None, rs13)
    assert rec.calls[-1] == ("single", R.ANTIALIAS)
    R.rasterize_gaussians(sc["means3D"], torch.zeros_like(sc["means3D"]), sc["shs"], None, sc["opacities"], sc["scales"],
                          sc["rotations"], None, rs, antialiasing=True)
    assert rec.calls[-1] == ("single", R.ANTIALIAS)
    R.rasterize_gaussians(sc["means3D"], torch.zeros_like(sc["means3D"]), sc["shs"], None, sc["opacities"], sc["scales"],
                          sc["rotations"], None, rs)
    assert rec.calls[-1] == ("single", 0)


def test_batch_sends_the_bit_and_rejects_mixed_settings(rec):
    sc, rs = _scene_and_settings()
    args = (sc["means3D"], None, sc["shs"], None, sc["opacities"], sc["scales"], sc["rotations"], None)
    rasterize_gaussians_batch(*args, [rs, rs])
    rasterize_gaussians_batch(*args, [rs, rs], antialiasing=True)
    rasterize_gaussians_batch(*args, [rs], activation_flags=R.ACT_OPACITY_SIGMOID, antialiasing=True)
    on = types.SimpleNamespace(**rs._asdict(), antialiasing=True)
    off = types.SimpleNamespace(**rs._asdict(), antialiasing=False)
    rasterize_gaussians_batch(*args, [on, on])
    assert [f for _, f in rec.calls] == [0, R.ANTIALIAS, R.ANTIALIAS | R.ACT_OPACITY_SIGMOID, R.ANTIALIAS]
    rasterize_gaussians_batch(*args, [on, on], antialiasing=False)                           # explicit choices win
    rasterize_gaussians_batch(*args, [rs], activation_flags=R.ANTIALIAS | R.ACT_SCALE_EXP, antialiasing=False)
    rasterize_gaussians_batch(*args, [rs], activation_flags=R.ANTIALIAS)
    assert [f for _, f in rec.calls[-3:]] == [0, R.ACT_SCALE_EXP, R.ANTIALIAS]
    with pytest.raises(ValueError):
        rasterize_gaussians_batch(*args, [on, off])
    with pytest.raises(ValueError):
        rasterize_gaussians_batch(*args, [rs, on])


class _Model:
    def __init__(self, sc):
        self.get_xyz, self.get_features = sc["means3D"], sc["shs"]
        self._opacity = torch.logit(sc["opacities"])
        self._scaling, self._rotation = torch.log(sc["scales"]), sc["rotations"]
        self.get_opacity, self.get_scaling, self.get_rotation = sc["opacities"], sc["scales"], sc["rotations"]
        self.active_sh_degree = self.max_sh_degree = sc["sh_degree"]


@pytest.mark.parametrize("fused", [False, True])
def test_render_reads_pipe_antialiasing(rec, fused):
    sc, _ = _scene_and_settings()
    pc, cam = _Model(sc), sc["cam"]
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    renderer.render(cam, pc, pipe, sc["bg"], fuse_activations=fused)
    pipe.antialiasing = False
    renderer.render(cam, pc, pipe, sc["bg"], fuse_activations=fused)
    pipe.antialiasing = True
    renderer.render(cam, pc, pipe, sc["bg"], fuse_activations=fused)
    kinds = {k for k, _ in rec.calls}
    assert kinds == ({"batch"} if fused else {"single"})
    assert [_aa(f) for _, f in rec.calls] == [False, False, True]
    if fused:
        assert rec.calls[-1][1] & R.ACT_OPACITY_SIGMOID


def test_render_views_renderer_and_animator_pass_the_switch(rec):
    sc, _ = _scene_and_settings()
    pc, cam = _Model(sc), sc["cam"]
    pipe = types.SimpleNamespace(antialiasing=True)
    renderer.render_views([cam, cam], pc, pipe, sc["bg"])
    assert rec.calls[-1][0] == "batch" and _aa(rec.calls[-1][1])
    renderer.render_views([cam, cam], pc, types.SimpleNamespace(), sc["bg"])
    assert not _aa(rec.calls[-1][1])
    rd = renderer.Renderer(pc, device="cpu")
    rd.render(cam)
    assert not _aa(rec.calls[-1][1])
    rd.render(cam, antialiasing=True)
    assert _aa(rec.calls[-1][1])
    from humangaussian_amd.animation import AvatarAnimator
    anim = AvatarAnimator(pc, types.SimpleNamespace(positions=lambda v: sc["means3D"]), device="cpu", antialiasing=True)
    anim.render_frame(None, cam)
    assert _aa(rec.calls[-1][1])
    anim = AvatarAnimator(pc, types.SimpleNamespace(positions=lambda v: sc["means3D"]), device="cpu")
    anim.render_frame(None, cam)
    assert not _aa(rec.calls[-1][1])
