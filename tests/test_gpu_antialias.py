"""The opt-in antialiasing filter (HGS_ANTIALIAS, ABI v17) on the device, against the fp64 reference of
tests/aa_reference.py with the parity suite's gates: images within 1e-4, gradients within 1e-3 max|g| with cosine above
1 - 1e-5.  Also: radii untouched by the filter, the stored opacity, the batch contract of test_gpu_batch.py with the
filter on, the packed backward, off-means-off, and what the filter is for (a coarse render that agrees with a
box-filtered fine one)."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import aa_reference
import oracle
from abi_runner import GEOM_DTYPE, RawCall, _p
from helpers import make_scene, oracle_settings
from humangaussian_amd import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians_batch, synth
from humangaussian_amd import rasterizer as R
from humangaussian_amd import renderer
from humangaussian_amd import view_parallel as vp
from oracle import gs_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("means3D", "shs", "opacities", "scales", "rotations")
IMG_TOL, GRAD_TOL, COS_TOL = 1e-4, 1e-3, 1e-5
# test 6: (alpha error with the filter) / (alpha error without it), 256^2 against a 4x4 pool of 1024^2, computed by the
# fp64 reference for aa_reference.FILTER_SCENE (aa_reference.filter_error_ratio_fp64(); test_antialias_cpu.py checks it)
FILTER_RATIO_FP64 = 0.19636


def _settings(sc, dev=DEV, mod=1.0, cam=None):
    cam = sc["cam"] if cam is None else cam
    return GaussianRasterizationSettings(cam.image_height, cam.image_width, math.tan(cam.FoVx * 0.5),
                                         math.tan(cam.FoVy * 0.5), sc["bg"].to(dev), mod,
                                         cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev),
                                         sc["sh_degree"], cam.camera_center.to(dev), False, False)


def _loss_weights(H, W, seed=0, B=None):
    g = torch.Generator().manual_seed(seed)
    lead = () if B is None else (B,)
    return [torch.randn(lead + s, generator=g) for s in ((3, H, W), (1, H, W), (1, H, W))]


def _zoomed_out(sh_degree=1):
    """small Gaussians seen from far away: most of them well below the 0.3 px^2 dilation"""
    return make_scene(P=800, sh_degree=sh_degree, seed=21, H=96, W=128, spread=0.5, scale=0.004, dist=6.0)


def _gate_images(got, ref, what):
    for name, x, y in zip(("color", "depth", "alpha"), got, ref):
        scale = max(1.0, float(y.abs().max())) if name == "depth" else 1.0
        err = float((x.detach().cpu().double() - y.detach().double()).abs().max())
        assert err <= IMG_TOL * scale, (what, name, err)


def _gate_grad(got, ref, what):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    scale = max(float(ref.abs().max()), 1e-12)
    err = float((got - ref).abs().max())
    assert err <= GRAD_TOL * scale, (what, err / scale)
    if float(ref.norm()) > 0:
        cos = float(torch.dot(got, ref) / (got.norm() * ref.norm()))
        assert cos >= 1 - COS_TOL, (what, cos)


def _hip(sc, aa, mod=1.0, colors_precomp=None, cov3D=None, weights=None, grads=True, **kw):
    """one view through GaussianRasterizer(antialiasing=aa); -> (color, radii, depth, alpha), grads dict"""
    rs = _settings(sc, mod=mod)
    ins = {k: sc[k].to(DEV).requires_grad_(grads) for k in ("means3D", "opacities")}
    if colors_precomp is None:
        ins["shs"] = sc["shs"].to(DEV).requires_grad_(grads)
    else:
        ins["colors_precomp"] = colors_precomp.to(DEV).requires_grad_(grads)
    if cov3D is None:
        ins["scales"] = sc["scales"].to(DEV).requires_grad_(grads)
        ins["rotations"] = sc["rotations"].to(DEV).requires_grad_(grads)
    else:
        ins["cov3D_precomp"] = cov3D.to(DEV).requires_grad_(grads)
    m2 = torch.zeros_like(ins["means3D"], requires_grad=grads)
    rast = GaussianRasterizer(rs, antialiasing=aa) if aa is not None else GaussianRasterizer(rs)
    out = rast(means3D=ins["means3D"], means2D=m2, opacities=ins["opacities"], shs=ins.get("shs"),
               colors_precomp=ins.get("colors_precomp"), scales=ins.get("scales"), rotations=ins.get("rotations"),
               cov3D_precomp=ins.get("cov3D_precomp"))
    if not grads:
        return out, None
    c, r, d, a = out
    wc, wd, wa = weights
    torch.autograd.backward([c, d, a], [wc.to(DEV), wd.to(DEV), wa.to(DEV)])
    g = {k: v.grad for k, v in ins.items()}
    g["means2D"] = m2.grad
    return (c.detach(), r, d.detach(), a.detach()), g


def _ref(sc, mod=1.0, colors_precomp=None, cov3D=None, weights=None):
    """fp64 AA reference with autograd; -> (color, radii, depth, alpha), grads dict"""
    st = oracle_settings(sc, scale_modifier=mod)
    ins = {k: sc[k].double().requires_grad_(True) for k in ("means3D", "opacities")}
    ins["shs"] = sc["shs"].double().requires_grad_(True) if colors_precomp is None else None
    ins["colors_precomp"] = None if colors_precomp is None else colors_precomp.double().requires_grad_(True)
    ins["scales"] = sc["scales"].double().requires_grad_(True) if cov3D is None else None
    ins["rotations"] = sc["rotations"].double().requires_grad_(True) if cov3D is None else None
    ins["cov3D_precomp"] = None if cov3D is None else cov3D.double().requires_grad_(True)
    m2 = torch.zeros(sc["means3D"].shape[0], 3, dtype=torch.float64, requires_grad=True)
    c, r, d, a = aa_reference.rasterize(ins["means3D"], m2, ins["shs"], ins["colors_precomp"], ins["opacities"],
                                        ins["scales"], ins["rotations"], ins["cov3D_precomp"], st, dtype=torch.float64)
    wc, wd, wa = weights
    ((c * wc.double()).sum() + (d * wd.double()).sum() + (a * wa.double()).sum()).backward()
    g = {k: v.grad for k, v in ins.items() if v is not None}
    g["means2D"] = m2.grad
    return (c.detach(), r, d.detach(), a.detach()), g


class _AARawCall(RawCall):
    """RawCall's forward through hgs_forward_batch_act with activation flags (the geom records are what we read)"""

    def forward_act(self, flags):
        lib, dev, P, H, W = self.lib, self.dev, self.P, self.H, self.W
        u8 = lambda n: torch.zeros(int(n), dtype=torch.uint8, device=dev)  # noqa: E731
        self.color = torch.zeros((3, H, W), device=dev)
        self.depth = torch.zeros((1, H, W), device=dev)
        self.alpha = torch.zeros((1, H, W), device=dev)
        self.radii = torch.full((P,), -7, dtype=torch.int32, device=dev)
        self.geom = u8(lib.hgs_geom_bytes(P, H, W))
        self.bin = u8(lib.hgs_bin_bytes(self.capacity))
        self.img = u8(lib.hgs_img_bytes(H, W))
        self.status_host = torch.zeros(8, dtype=torch.int32).pin_memory()
        stream = torch.cuda.current_stream(dev)
        rc = lib.hgs_forward_batch_act(ctypes.byref(self.settings), 1, P, self.M, _p(self.means3D), _p(self.shs),
                                       _p(self.colors_precomp), _p(self.opac), _p(self.scales), _p(self.rots),
                                       _p(self.cov3D), _p(self.color), _p(self.depth), _p(self.alpha), _p(self.radii),
                                       _p(self.geom), _p(self.bin), self.capacity, _p(self.img), 1, 0,
                                       ctypes.c_void_p(self.status_host.data_ptr()), 0, None, None, flags,
                                       ctypes.c_void_p(stream.cuda_stream))
        stream.synchronize()
        self.status = [int(x) & 0xFFFFFFFF for x in self.status_host.tolist()]
        return rc


def _fp32_rho_opacity(sc):
    """opacity * rho in fp32 with the kernel's operations: a0, b, c0 from the oracle's fp32 projection without the
    dilation (LOWPASS = 0: `expr + 0.0` is `expr`), det from the dilated one"""
    args = (sc["means3D"], None, sc["shs"], None, sc["opacities"], sc["scales"], sc["rotations"], None, oracle_settings(sc))
    pre = gs_oracle.preprocess(*args)
    saved = gs_oracle.LOWPASS
    gs_oracle.LOWPASS = 0.0
    try:
        pre0 = gs_oracle.preprocess(*args)
    finally:
        gs_oracle.LOWPASS = saved
    a, b, c = pre["cov2D"].unbind(1)
    a0, b0, c0 = pre0["cov2D"].unbind(1)
    assert torch.equal(b, b0)
    det = a * c - b * b
    ratio = (a0 * c0 - b * b) / det
    rho = torch.sqrt(torch.clamp(ratio, min=aa_reference.MIN_RATIO))
    return pre["opacity"] * rho, pre["visible"], pre["conic"]


# ---------------------------------------------------------------------------------------------- 1. forward parity
@pytest.mark.parametrize("case", ["deg0", "deg3", "zoomed_out"])
def test_forward_parity(case):
    sc = {"deg0": lambda: make_scene(P=600, sh_degree=0, seed=1, H=80, W=112, spread=0.35),
          "deg3": lambda: make_scene(P=600, sh_degree=3, seed=2, H=80, W=112, spread=0.35),
          "zoomed_out": _zoomed_out}[case]()
    w = _loss_weights(sc["cam"].image_height, sc["cam"].image_width)
    (c, r, d, a), _ = _hip(sc, True, weights=w, grads=False)
    (c0, r0, d0, a0), _ = _hip(sc, None, weights=w, grads=False)
    assert torch.equal(r, r0), "the filter changed radii"
    with torch.no_grad():
        ref = aa_reference.rasterize(sc["means3D"].double(), None, sc["shs"].double(), None, sc["opacities"].double(),
                                     sc["scales"].double(), sc["rotations"].double(), None, oracle_settings(sc),
                                     dtype=torch.float64)
    assert torch.equal(r.cpu(), ref[1])
    _gate_images((c, d, a), (ref[0], ref[2], ref[3]), case)
    assert float((a.cpu() - a0.cpu()).abs().max()) > 1e-3           # the filter changes the image
    # the stored record: op = fp32 opacity * rho within 2 ulp; the rest of the record as without the filter
    rc_on, rc_off = _AARawCall(sc), _AARawCall(sc)
    assert rc_on.forward_act(R.ANTIALIAS) == 0 and rc_off.forward_act(0) == 0
    g_on, g_off = rc_on.geom_records(), rc_off.geom_records()
    want, vis, conic = _fp32_rho_opacity(sc)
    # (where the oracle's fp32 projection reproduces the kernel's conic bit for bit - nearly everywhere - its a0, b, c0
    # are the kernel's too, and rho is compared at the last bits)
    same = vis.numpy() & np.all(np.stack([g_on[f] for f in ("ca", "cb", "cc")], 1) == conic.numpy(), axis=1)
    assert same.sum() >= 0.9 * vis.numpy().sum(), (int(same.sum()), int(vis.sum()))
    got = g_on["op"][same].astype(np.float32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.numpy()[same].astype(np.float32).view(np.int32).astype(np.int64))
    assert int(ulp.max()) <= 2, int(ulp.max())
    # ... radii, tile rects (so tiles_touched and the entry ids) and the number of list entries included
    for f in ("mx", "my", "ca", "cb", "cc", "depth", "radius", "r", "g", "b", "rect_lo", "rect_hi", "offset", "clamped",
              "flags"):
        assert np.array_equal(g_on[f], g_off[f]), f
    assert rc_on.status[0] == rc_off.status[0] > 0, (rc_on.status, rc_off.status)
    if case == "zoomed_out":
        with torch.no_grad():
            pre = aa_reference.preprocess_aa(sc["means3D"].double(), None, sc["shs"].double(), None,
                                             sc["opacities"].double(), sc["scales"].double(), sc["rotations"].double(),
                                             None, oracle_settings(sc), dtype=torch.float64)
        med = float(pre["rho"][pre["visible"]].median())
        assert med < 0.5, med


# ---------------------------------------------------------------------------------------------- 2. backward parity
def _check_backward(sc, what, **kw):
    H, W = sc["cam"].image_height, sc["cam"].image_width
    w = _loss_weights(H, W, seed=3)
    hip_out, hg = _hip(sc, True, weights=w, **kw)
    ref_out, rg = _ref(sc, weights=w, **kw)
    assert torch.equal(hip_out[1].cpu(), ref_out[1])
    _gate_images((hip_out[0], hip_out[2], hip_out[3]), (ref_out[0], ref_out[2], ref_out[3]), what)
    for k in rg:                          # (scales at scale_modifier != 1: the fork's dL/d(mod * scale), like the oracle)
        _gate_grad(hg[k], rg[k], (what, k))
    return hg, rg


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_backward_parity_sh_degrees(deg):
    _check_backward(make_scene(P=500, sh_degree=deg, seed=10 + deg, H=64, W=80, spread=0.3), f"deg{deg}")


def test_backward_parity_zoomed_out():
    _check_backward(_zoomed_out(), "zoomed_out")


def test_backward_parity_precomputed_colours_and_covariances():
    sc = make_scene(P=500, sh_degree=1, seed=30, H=64, W=80, spread=0.3)
    g = torch.Generator().manual_seed(4)
    cols = torch.rand(500, 3, generator=g)
    from helpers import cov3d_from
    _check_backward(sc, "colors_precomp", colors_precomp=cols)
    _check_backward(sc, "cov3D_precomp", cov3D=cov3d_from(sc))


def test_backward_parity_scale_modifier_both_conventions():
    sc = make_scene(P=500, sh_degree=2, seed=31, H=64, W=80, spread=0.3)
    hg, rg = _check_backward(sc, "mod0.7", mod=0.7)
    # the true derivative on request (GRAD_SCALE_TRUE_DERIVATIVE), through the batched entry point
    H, W = sc["cam"].image_height, sc["cam"].image_width
    wc, wd, wa = _loss_weights(H, W, seed=3)
    ins = {k: sc[k].to(DEV).requires_grad_(True) for k in NAMES}
    m2 = torch.zeros((1,) + tuple(ins["means3D"].shape), device=DEV, requires_grad=True)
    c, r, d, a = rasterize_gaussians_batch(ins["means3D"], m2, ins["shs"], None, ins["opacities"], ins["scales"],
                                           ins["rotations"], None, [_settings(sc, mod=0.7)],
                                           activation_flags=R.GRAD_SCALE_TRUE_DERIVATIVE, antialiasing=True)
    torch.autograd.backward([c, d, a], [wc[None].to(DEV), wd[None].to(DEV), wa[None].to(DEV)])
    _gate_grad(ins["scales"].grad, rg["scales"] * 0.7, "true derivative")      # dL/dscale = mod * dL/d(mod * scale)
    assert torch.equal(ins["means3D"].grad, hg["means3D"])


def test_backward_parity_fused_activations():
    sc = make_scene(P=500, sh_degree=1, seed=32, H=64, W=80, spread=0.3)
    H, W = sc["cam"].image_height, sc["cam"].image_width
    wc, wd, wa = _loss_weights(H, W, seed=5)
    g = torch.Generator().manual_seed(6)
    raw = dict(means3D=sc["means3D"], shs=sc["shs"], opacities=torch.logit(sc["opacities"]),
               scales=torch.log(sc["scales"]), rotations=sc["rotations"] * (0.5 + torch.rand(500, 1, generator=g)))
    ins = {k: v.to(DEV).requires_grad_(True) for k, v in raw.items()}
    m2 = torch.zeros((1,) + tuple(ins["means3D"].shape), device=DEV, requires_grad=True)
    c, r, d, a = rasterize_gaussians_batch(ins["means3D"], m2, ins["shs"], None, ins["opacities"], ins["scales"],
                                           ins["rotations"], None, [_settings(sc)],
                                           activation_flags=R.ACT_OPACITY_SIGMOID | R.ACT_SCALE_EXP | R.ACT_ROTATION_NORMALIZE,
                                           antialiasing=True)
    torch.autograd.backward([c, d, a], [wc[None].to(DEV), wd[None].to(DEV), wa[None].to(DEV)])
    ref = {k: v.double().requires_grad_(True) for k, v in raw.items()}
    om2 = torch.zeros(500, 3, dtype=torch.float64, requires_grad=True)
    oc, orad, od, oa = aa_reference.rasterize(ref["means3D"], om2, ref["shs"], None, torch.sigmoid(ref["opacities"]),
                                              torch.exp(ref["scales"]),
                                              torch.nn.functional.normalize(ref["rotations"], dim=1), None,
                                              oracle_settings(sc), dtype=torch.float64)
    ((oc * wc.double()).sum() + (od * wd.double()).sum() + (oa * wa.double()).sum()).backward()
    _gate_images((c[0], d[0], a[0]), (oc, od, oa), "fused")
    for k in NAMES:
        _gate_grad(ins[k].grad, ref[k].grad, ("fused", k))
    _gate_grad(m2.grad[0], om2.grad, ("fused", "means2D"))


# ---------------------------------------------------------------------------------------------- 3. batch contract
def _cams(n, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        r = torch.rand(4, generator=g).tolist()
        out.append(synth.orbit_camera(-30 + 60 * r[0], -180 + 360 * (i + r[1]) / n, 1.5 + 1.5 * r[2], 40 + 30 * r[3], H, W))
    return out


# SH 3: the one-view form (B = 1), the view-parallel form (2..8) and the loop (16: d3, the run-time switch); SH 2 at 16
# views: the loop's compile-time copy d2_aa
@pytest.mark.parametrize("B,deg", [(1, 3), (2, 3), (3, 3), (8, 3), (16, 3), (16, 2)])
def test_batch_equals_single_view_calls_bitwise(B, deg):
    H, W, P = 48, 64, 700
    sc = make_scene(P=P, sh_degree=deg, seed=40 + B + deg, H=H, W=W, spread=0.3, scale=0.02)
    cams = _cams(B, H, W, seed=B)
    rsl = [_settings(sc, cam=cm) for cm in cams]
    wc, wd, wa = (t.to(DEV) for t in _loss_weights(H, W, seed=B, B=B))
    ins = {k: sc[k].to(DEV).requires_grad_(True) for k in NAMES}
    m2 = torch.zeros((B,) + tuple(ins["means3D"].shape), device=DEV, requires_grad=True)
    c, r, d, a = rasterize_gaussians_batch(ins["means3D"], m2, ins["shs"], None, ins["opacities"], ins["scales"],
                                           ins["rotations"], None, rsl, antialiasing=True)
    torch.autograd.backward([c, d, a], [wc, wd, wa])
    acc = None
    for b in range(B):
        si = {k: sc[k].to(DEV).requires_grad_(True) for k in NAMES}
        sm2 = torch.zeros_like(si["means3D"], requires_grad=True)
        cb, rb, db, ab = GaussianRasterizer(rsl[b], antialiasing=True)(
            means3D=si["means3D"], means2D=sm2, shs=si["shs"], opacities=si["opacities"], scales=si["scales"],
            rotations=si["rotations"])
        torch.autograd.backward([cb, db, ab], [wc[b], wd[b], wa[b]])
        for x, y, name in ((c[b], cb, "color"), (r[b], rb, "radii"), (d[b], db, "depth"), (a[b], ab, "alpha"),
                           (m2.grad[b], sm2.grad, "means2D")):
            assert torch.equal(x, y), (B, b, name)
        gb = {k: si[k].grad for k in NAMES}
        acc = gb if acc is None else {k: acc[k] + gb[k] for k in NAMES}
    for k in NAMES:
        assert torch.equal(ins[k].grad, acc[k]), (B, k, float((ins[k].grad - acc[k]).abs().max()))
    assert float(ins["opacities"].grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- 4. packed backward
@pytest.mark.parametrize("fused", [False, True])
def test_packed_backward_equals_unpacked_plus_pack(fused):
    sc = make_scene(P=600, sh_degree=1, seed=50, H=64, W=80, spread=0.3, scale=0.02)
    H, W = sc["cam"].image_height, sc["cam"].image_width
    wc, wd, wa = (t.to(DEV) for t in _loss_weights(H, W, seed=7))
    act = (R.ACT_OPACITY_SIGMOID | R.ACT_SCALE_EXP | R.ACT_ROTATION_NORMALIZE) if fused else 0
    src = dict(sc) if not fused else dict(sc, opacities=torch.logit(sc["opacities"]), scales=torch.log(sc["scales"]))

    def run(packed):
        ins = {k: src[k].to(DEV).requires_grad_(True) for k in NAMES}
        m2 = torch.zeros((1,) + tuple(ins["means3D"].shape), device=DEV, requires_grad=True)
        c, r, d, a = rasterize_gaussians_batch(ins["means3D"], m2, ins["shs"], None, ins["opacities"], ins["scales"],
                                               ins["rotations"], None, [_settings(sc)], activation_flags=act,
                                               antialiasing=True)
        tens = [ins[k] for k in NAMES] + [m2]
        if not packed:
            return torch.autograd.grad([c, d, a], tens, [wc[None], wd[None], wa[None]]), r[0], None
        with R.packed_gradients() as pg:
            gl = torch.autograd.grad([c, d, a], tens, [wc[None], wd[None], wa[None]])
            pack = pg.take()
        return gl, r[0], pack
    gl, radii, _ = run(False)
    gp, radii_p, pack = run(True)
    assert pack is not None
    assert torch.equal(radii, radii_p)
    grads = dict(zip(NAMES, gl))
    grads["means2D"] = gl[-1][0]
    want = vp.pack_contribution(grads, radii)
    assert torch.equal(pack, want), float((pack - want).abs().max())
    for k, x, y in zip(NAMES, gl, gp):
        assert torch.equal(x, y), k


def _aa_render_fn(cam, leaves, means2D, bg, sh_degree):
    """a custom render_fn with the filter on"""
    rs = GaussianRasterizationSettings(
        int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0,
        cam.world_view_transform, cam.full_proj_transform, sh_degree, cam.camera_center, False, False)
    return GaussianRasterizer(rs, antialiasing=True)(means3D=leaves["means3D"], means2D=means2D, shs=leaves["shs"],
                                                     opacities=leaves["opacities"], scales=leaves["scales"],
                                                     rotations=leaves["rotations"])


def test_view_parallel_step_with_an_antialiased_render_fn_equals_the_serial_loop():
    H, W, n = 48, 64, 3
    sc = make_scene(P=500, sh_degree=1, seed=60, H=H, W=W, spread=0.3, scale=0.02)
    cams = [types.SimpleNamespace(image_height=cm.image_height, image_width=cm.image_width, FoVx=cm.FoVx, FoVy=cm.FoVy,
                                  world_view_transform=cm.world_view_transform.to(DEV),
                                  full_proj_transform=cm.full_proj_transform.to(DEV),
                                  camera_center=cm.camera_center.to(DEV)) for cm in _cams(n, H, W, seed=9)]
    params = {k: sc[k].to(DEV) for k in NAMES}
    bg = sc["bg"].to(DEV)
    ws = [[t.to(DEV) for t in _loss_weights(H, W, seed=100 + v)] for v in range(n)]

    def loss_grad(v, c, d, a):
        return tuple(ws[v])
    grads, radii, _ = vp.render_views_parallel(cams, params, bg, 1, loss_grad, render_fn=_aa_render_fn, pipeline=True)
    L = {k: params[k].detach().requires_grad_(True) for k in NAMES}
    acc, rmax = None, None
    for v in range(n):
        m2 = torch.zeros_like(L["means3D"], requires_grad=True)
        c, r, d, a = _aa_render_fn(cams[v], L, m2, bg, 1)
        gl = torch.autograd.grad([c, d, a], [L[k] for k in NAMES] + [m2], ws[v])
        g = dict(zip(NAMES + ("means2D",), gl))
        acc = g if acc is None else {k: acc[k] + g[k] for k in g}
        rmax = r if rmax is None else torch.maximum(rmax, r)
    assert torch.equal(radii, rmax)
    for k in vp.GRAD_KEYS:
        assert torch.equal(grads[k].reshape(acc[k].shape), acc[k]), k
    # ... and under a packed-gradients request the same function gets the packed AA backward: the same bits
    m2 = torch.zeros_like(L["means3D"], requires_grad=True)
    c, r, d, a = _aa_render_fn(cams[0], L, m2, bg, 1)
    gl = torch.autograd.grad([c, d, a], [L[k] for k in NAMES] + [m2], ws[0])
    m2p = torch.zeros_like(L["means3D"], requires_grad=True)
    cp, rp, dp, ap = _aa_render_fn(cams[0], L, m2p, bg, 1)
    assert torch.equal(rp, r)
    with R.packed_gradients() as pg:
        torch.autograd.grad([cp, dp, ap], [L[k] for k in NAMES] + [m2p], ws[0])
        pack = pg.take()
    g = dict(zip(NAMES + ("means2D",), gl))
    assert pack is not None and torch.equal(pack, vp.pack_contribution(g, r))


# ---------------------------------------------------------------------------------------------- 5. off means off
def test_off_means_off():
    sc = make_scene(P=600, sh_degree=2, seed=70, H=64, W=80, spread=0.3)
    w = _loss_weights(64, 80, seed=8)
    o_none, g_none = _hip(sc, None, weights=w)
    o_off, g_off = _hip(sc, False, weights=w)
    for x, y in zip(o_none, o_off):
        assert torch.equal(x, y)
    for k in g_none:
        assert torch.equal(g_none[k], g_off[k]), k

    class Model:
        get_xyz, get_features = sc["means3D"].to(DEV), sc["shs"].to(DEV)
        get_opacity, get_scaling, get_rotation = sc["opacities"].to(DEV), sc["scales"].to(DEV), sc["rotations"].to(DEV)
        active_sh_degree = max_sh_degree = 2
    cm = sc["cam"]
    cam = types.SimpleNamespace(image_height=cm.image_height, image_width=cm.image_width, FoVx=cm.FoVx, FoVy=cm.FoVy,
                                world_view_transform=cm.world_view_transform.to(DEV),
                                full_proj_transform=cm.full_proj_transform.to(DEV), camera_center=cm.camera_center.to(DEV))
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    (c0, r0, d0, a0), _ = _hip(sc, None, grads=False)
    out = renderer.render(cam, Model(), pipe, sc["bg"].to(DEV))
    assert torch.equal(out["render"], c0) and torch.equal(out["alpha_3dgs"], a0) and torch.equal(out["radii"], r0)
    pipe.antialiasing = True
    out_aa = renderer.render(cam, Model(), pipe, sc["bg"].to(DEV))
    (c_aa, *_), _ = _hip(sc, True, grads=False)
    assert torch.equal(out_aa["render"], c_aa) and not torch.equal(out_aa["render"], c0)


# ---------------------------------------------------------------------------------------------- 6. what it is for
def test_coarse_render_matches_the_box_filtered_fine_one():
    errs = {}
    for aa in (False, True):
        alphas = []
        for H in (aa_reference.FILTER_HI, aa_reference.FILTER_LO):
            sc = aa_reference.filter_scene(H)
            (_, _, _, a), _ = _hip(sc, aa, grads=False)
            alphas.append(a.cpu())
        errs[aa] = aa_reference.pooled_alpha_error(*alphas)
    ratio = errs[True] / errs[False]
    assert ratio <= FILTER_RATIO_FP64 * 1.05 + 0.005, (ratio, errs)


def test_off_path_equals_the_parent_commit():
    """the filter off, bit for bit as the build before it (tests/golden/make_aa_off_fixture.py: fingerprints of the
    outputs and gradients of three calls, recorded with that build)"""
    import importlib.util
    import json
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_aa_off_fixture", os.path.join(golden, "make_aa_off_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(os.path.join(golden, "aa_off_parent.json")))
    got = gen.fingerprints()
    assert sorted(got) == sorted(want)
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, differ
