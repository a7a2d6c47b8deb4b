"""render_views_parallel on the HIP path, in one process (world 1, no process group), against two plain references:

A. the SAME render function on the device, outside any `packed_gradients()` request: per-view `torch.autograd.grad` on the
   leaves, summed in view order, radii max over the views - bit for bit for the serial modes (pipelined rounds, and the
   local sum of pipeline=False), to rounding for `batched=True`;
B. the fp64 oracle on the CPU inside the same render function (activations / transforms in fp64): within GRAD_TOL of
   max|g| per tensor, as in tests/test_gpu_parity.py.

The render functions are the ones a caller of the step writes: the default HIP rasterizer; raw parameters through
sigmoid / exp / normalize (by hand, and through `renderer.render` on a GaussianModel-shaped object); re-posed means; a
subset of the Gaussians; two rasterizer calls per view; precomputed colours; a custom `render_batch_fn`.  The step may
take the gradient pack the rasterizer's backward writes (`rasterizer.packed_gradients`) only for the default functions:
that pack holds the gradients w.r.t. the rasterizer's inputs, which for any other function are not the leaves.

The last tests hold the packed-gradients request itself to its contract: nestable, one pack per request only when one
rasterizer backward ran, a pack that does not fit the leaves refused by the step, and the gradients autograd receives
unchanged by the request."""
import math
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

import oracle
from helpers import make_scene
from humangaussian_amd import rasterizer as R
from humangaussian_amd import renderer, synth
from humangaussian_amd import view_parallel as vp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAD_TOL = 1e-3           # of max|g| per tensor, vs the fp64 oracle (tests/test_gpu_parity.py)
BATCH_TOL = 1e-5          # batched=True vs the serial loop, of max|g| (the bound of tests/test_view_parallel_cpu.py)
NAMES = ("means3D", "shs", "opacities", "scales", "rotations")
NUM_VIEWS = 5

# (P, sh_degree, H = W, seed): SH degree 1 and 3
SCENES = {"deg1": (1500, 1, 64, 21), "deg3": (2500, 3, 96, 22)}


# ------------------------------------------------------------------------------------------- scenes and cameras
@lru_cache(maxsize=None)
def _scene(name):
    P, deg, H, seed = SCENES[name]
    sc = make_scene(P=P, sh_degree=deg, seed=seed, H=H, W=H, spread=0.3, scale=0.05)
    g = torch.Generator().manual_seed(seed + 1)
    act = {k: sc[k] for k in NAMES}
    # the model's raw parameters behind the same activated values (GaussianModel: _opacity logits, _scaling log-scales,
    # un-normalised _rotation)
    raw = dict(act, opacities=torch.logit(sc["opacities"]), scales=torch.log(sc["scales"]),
               rotations=sc["rotations"] * (0.5 + 1.5 * torch.rand(P, 1, generator=g)))
    cams = [synth.orbit_camera(8.0 * (v - 2), 360.0 / NUM_VIEWS * v + 10.0, 2.0, 50.0, H, H) for v in range(NUM_VIEWS)]
    return SimpleNamespace(P=P, deg=deg, H=H, bg=sc["bg"], act=act, raw=raw, cams=cams,
                           dcams=[_to(c, DEV) for c in cams])


def _to(cam, dev):
    return cam._replace(world_view_transform=cam.world_view_transform.to(dev),
                        full_proj_transform=cam.full_proj_transform.to(dev), camera_center=cam.camera_center.to(dev))


def _loss_grad(v, color, depth, alpha):
    """seeded per view; drawn in fp32 so that the fp64 reference gets the very same incoming gradients"""
    g = torch.Generator().manual_seed(100 + v)
    return tuple(torch.randn(t.shape, generator=g).to(t.device, t.dtype) for t in (color, depth, alpha))


# ------------------------------------------------------------------------------------------- rasterizer primitives
def _hip_settings(cam, bg, deg):
    return R.GaussianRasterizationSettings(int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5),
                                           math.tan(cam.FoVy * 0.5), bg, 1.0, cam.world_view_transform,
                                           cam.full_proj_transform, deg, cam.camera_center, False, False)


def _hip_raster(cam, bg, deg, m3, m2, shs, cp, op, sc, ro):
    return R.GaussianRasterizer(_hip_settings(cam, bg, deg))(means3D=m3, means2D=m2, shs=shs, colors_precomp=cp,
                                                             opacities=op, scales=sc, rotations=ro)


def _oracle_raster(cam, bg, deg, m3, m2, shs, cp, op, sc, ro):
    st = oracle.OracleSettings(int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5),
                               math.tan(cam.FoVy * 0.5), bg, 1.0, cam.world_view_transform, cam.full_proj_transform, deg,
                               cam.camera_center, False, False)
    return oracle.rasterize(m3, m2, shs, cp, op, sc, ro, None, st, dtype=torch.float64)


# ------------------------------------------------------------------------------------------- render functions
_REPOSE_A = ((0.9, -0.2, 0.1), (0.15, 1.1, 0.05), (-0.1, 0.08, 0.95))
_REPOSE_T = (0.05, -0.03, 0.02)


def _render_fns(raster):
    """name -> render_fn (camera, leaves, means2D, bg, sh_degree) built on `raster` (HIP or fp64 oracle)"""
    def plain(cam, L, m2, bg, deg):
        return raster(cam, bg, deg, L["means3D"], m2, L["shs"], None, L["opacities"], L["scales"], L["rotations"])

    def act(cam, L, m2, bg, deg):                                        # raw parameters through the activations
        return raster(cam, bg, deg, L["means3D"], m2, L["shs"], None, torch.sigmoid(L["opacities"]),
                      torch.exp(L["scales"]), torch.nn.functional.normalize(L["rotations"]))

    def repose(cam, L, m2, bg, deg):                                     # an affine map of the means
        x = L["means3D"]
        A, t = x.new_tensor(_REPOSE_A), x.new_tensor(_REPOSE_T)
        return raster(cam, bg, deg, x @ A.T + t, m2, L["shs"], None, L["opacities"], L["scales"], L["rotations"])

    def subset(cam, L, m2, bg, deg):                                     # two Gaussians of three
        P = L["means3D"].shape[0]
        idx = torch.arange(P, device=L["means3D"].device)
        idx = idx[idx % 3 != 1]
        c, r, d, a = raster(cam, bg, deg, L["means3D"][idx], m2[idx], L["shs"][idx], None, L["opacities"][idx],
                            L["scales"][idx], L["rotations"][idx])
        full = torch.zeros(P, dtype=r.dtype, device=r.device)
        full[idx] = r
        return c, full, d, a

    def twice(cam, L, m2, bg, deg):                                      # two rasterizer calls, summed
        c1, r1, d1, a1 = plain(cam, L, m2, bg, deg)
        c2, r2, d2, a2 = plain(cam, L, m2, 1.0 - bg, deg)
        return c1 + c2, torch.maximum(r1, r2), d1 + d2, a1 + a2

    def precomp(cam, L, m2, bg, deg):                                    # colours precomputed (not eligible for the pack)
        return raster(cam, bg, deg, L["means3D"], m2, None, torch.sigmoid(L["shs"][:, 0]), L["opacities"], L["scales"],
                      L["rotations"])

    return {"default": plain, "act_hand": act, "repose": repose, "subset": subset, "twice": twice, "precomp": precomp}


class _StandInModel:
    """GaussianModel-shaped (scene/gaussian_model.py's getters): raw tensors in, activated values out."""

    def __init__(self, L, deg):
        self._xyz, self._features, self._opacity, self._scaling, self._rotation = (
            L["means3D"], L["shs"], L["opacities"], L["scales"], L["rotations"])
        self.active_sh_degree = self.max_sh_degree = deg

    get_xyz = property(lambda self: self._xyz)
    get_features = property(lambda self: self._features)
    get_opacity = property(lambda self: torch.sigmoid(self._opacity))
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))


_PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def _act_renderer_fn(cam, L, m2, bg, deg):
    """HumanGaussian's own `render()` (renderer.render, activations un-fused) on a stand-in model; the step's means2D is
    handed in as the screen-space leaf render() would create for itself"""
    saved = renderer._screenspace_points
    renderer._screenspace_points = lambda xyz, views=None: (m2, False)
    try:
        out = renderer.render(cam, _StandInModel(L, deg), _PIPE, bg, fuse_activations=False)
    finally:
        renderer._screenspace_points = saved
    return out["render"], out["radii"], out["depth_3dgs"], out["alpha_3dgs"]


def _act_batch_fn(cams, L, m2, bg, deg):
    """custom render_batch_fn: the rank's views in one batched call, activations applied in torch"""
    return R.rasterize_gaussians_batch(L["means3D"], m2, L["shs"], None, torch.sigmoid(L["opacities"]),
                                       torch.exp(L["scales"]), torch.nn.functional.normalize(L["rotations"]), None,
                                       [_hip_settings(c, bg, deg) for c in cams])


HIP_FNS = dict(_render_fns(_hip_raster), default=vp.hip_render_fn, act_renderer=_act_renderer_fn)
ORACLE_FNS = dict(_render_fns(_oracle_raster))
ORACLE_FNS["act_renderer"] = ORACLE_FNS["act_hand"]
RAW = ("act_hand", "act_renderer")                 # the functions that take the model's raw parameters
CASES = [(s, f) for s in SCENES for f in ("default", "act_hand", "act_renderer", "repose", "subset", "twice", "precomp")]


def _params(s, fn, dtype, dev):
    src = s.raw if fn in RAW else s.act
    return {k: src[k].to(dev, dtype) for k in NAMES}


# ------------------------------------------------------------------------------------------- the two references
def _serial(render_fn, cams, params, bg, deg):
    """per-view autograd on the leaves, no packed request: -> [(grads dict, radii)] per view"""
    L = {k: params[k].detach().requires_grad_(True) for k in NAMES}
    out = []
    for v, cam in enumerate(cams):
        m2 = torch.zeros_like(L["means3D"], requires_grad=True)
        c, r, d, a = render_fn(cam, L, m2, bg, deg)
        gl = torch.autograd.grad([c, d, a], [L[k] for k in NAMES] + [m2], _loss_grad(v, c, d, a), allow_unused=True)
        tens = list(L.values()) + [m2]
        out.append(({k: (g if g is not None else torch.zeros_like(t)) for k, g, t in zip(NAMES + ("means2D",), gl, tens)},
                    r))
    return out


def _prefix(per_view, n):
    """the serial loop's accumulation over the first n views, in view order"""
    g, r = dict(per_view[0][0]), per_view[0][1]
    for gv, rv in per_view[1:n]:
        g = {k: g[k] + gv[k] for k in g}
        r = torch.maximum(r, rv)
    return g, r


@lru_cache(maxsize=None)
def _ref_a(scene, fn):
    s = _scene(scene)
    return _serial(HIP_FNS[fn], s.dcams, _params(s, fn, torch.float32, DEV), s.bg.to(DEV), s.deg)


@lru_cache(maxsize=None)
def _ref_b(scene, fn):
    s = _scene(scene)
    return _serial(ORACLE_FNS[fn], s.cams, _params(s, fn, torch.float64, "cpu"), s.bg.double(), s.deg)


class _TakeLog:
    """records what `packed_gradients.take()` handed the step (None or a pack)"""

    def __init__(self, monkeypatch, alter=None):
        self.taken = []
        real = R.packed_gradients.take

        def take():
            p = real()
            if alter is not None and p is not None:
                p = alter(p)
            self.taken.append(p)
            return p
        monkeypatch.setattr(R.packed_gradients, "take", staticmethod(take))


def _run(scene, fn, n, **kw):
    s = _scene(scene)
    params = _params(s, fn, torch.float32, DEV)
    grads, radii, outs = vp.render_views_parallel(s.dcams[:n], params, s.bg.to(DEV), s.deg, _loss_grad,
                                                  render_fn=HIP_FNS[fn], **kw)
    assert [v for v, *_ in outs] == list(range(n))
    return grads, radii


def _check_bits(got, ref, what):
    g, r = got
    gr, rr = ref
    assert torch.equal(r, rr), (what, "radii")
    for k in vp.GRAD_KEYS:
        assert g[k].shape == gr[k].shape, (what, k, tuple(g[k].shape))
        assert torch.equal(g[k], gr[k]), (what, k, float((g[k] - gr[k]).abs().max()))


def _check_rounding(got, ref, what):
    g, r = got
    gr, rr = ref
    assert torch.equal(r, rr), (what, "radii")
    for k in vp.GRAD_KEYS:
        scale = max(float(gr[k].abs().max()), 1e-30)
        assert float((g[k].double() - gr[k].double()).abs().max()) <= BATCH_TOL * scale, (what, k)


def _check_fp64(got, ref, what):
    g, gr = got[0], ref[0]          # (radii: against reference A, whose rasterizer rounds like this one)
    for k in vp.GRAD_KEYS:
        ref64 = gr[k]
        scale = max(float(ref64.abs().max()), 1e-12)
        err = float((g[k].cpu().double() - ref64).abs().max())
        assert err <= GRAD_TOL * scale, (what, k, err / scale)


def _assert_pack_use(log, fn, calls):
    if fn == "default":            # the default path keeps the pack its backward wrote
        assert len(log.taken) == calls and all(p is not None for p in log.taken), (fn, log.taken)
    else:                          # any other function: no request, its autograd result is packed
        assert log.taken == [], (fn, len(log.taken))


# ------------------------------------------------------------------------------------------- the matrix
MODES = [  # (name, views, keyword arguments, packed backwards of a default step)
    ("one_view", 1, dict(pipeline=False), 1),
    ("one_view_scatter", 1, dict(pipeline=False, collective="scatter"), 1),
    ("rounds_3", 3, dict(pipeline=None), 3),
    ("rounds_5", 5, dict(pipeline=True), 5),
    ("local_sum_3", 3, dict(pipeline=False), 3),
    ("local_sum_3_scatter", 3, dict(pipeline=False, collective="scatter"), 3),
]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scene,fn", CASES, ids=[f"{s}-{f}" for s, f in CASES])
def test_view_parallel_step_equals_the_serial_loop_and_the_fp64_oracle(monkeypatch, scene, fn):
    """Every mode of the one-view-at-a-time step is the serial loop's accumulation bit for bit (reference A), and within
    GRAD_TOL of the fp64 oracle run through the same render function (reference B)."""
    ref_a, ref_b = _ref_a(scene, fn), _ref_b(scene, fn)
    for name, n, kw, calls in MODES:
        log = _TakeLog(monkeypatch)
        got = _run(scene, fn, n, **kw)
        what = (scene, fn, name)
        _check_bits(got, _prefix(ref_a, n), what)
        _check_fp64(got, _prefix(ref_b, n), what)
        _assert_pack_use(log, fn, calls)


BATCH_CASES = [(s, f) for s in SCENES for f in ("default", "act_batch")]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scene,fn", BATCH_CASES, ids=[f"{s}-{f}" for s, f in BATCH_CASES])
@pytest.mark.parametrize("collective", ["allgather", "scatter"])
def test_batched_step_equals_the_serial_loop_and_the_fp64_oracle(monkeypatch, scene, fn, collective):
    """batched=True (the rank's views in ONE batched call): the serial loop's values to rounding (reference A, the per-view
    render function that matches the batch function), within GRAD_TOL of the fp64 oracle (reference B)."""
    s = _scene(scene)
    single = "default" if fn == "default" else "act_hand"
    params = _params(s, single, torch.float32, DEV)
    for n in (3, NUM_VIEWS):
        log = _TakeLog(monkeypatch)
        kw = dict(batched=True, collective=collective)
        if fn != "default":
            kw["render_batch_fn"] = _act_batch_fn
        grads, radii, outs = vp.render_views_parallel(s.dcams[:n], params, s.bg.to(DEV), s.deg, _loss_grad, **kw)
        assert [v for v, *_ in outs] == list(range(n))
        what = (scene, fn, collective, n)
        _check_rounding((grads, radii), _prefix(_ref_a(scene, single), n), what)
        _check_fp64((grads, radii), _prefix(_ref_b(scene, single), n), what)
        _assert_pack_use(log, fn, 1)


# ------------------------------------------------------------------------------------------- the packed request
def _one_backward(s, fn="default", cam=0):
    """one view of HIP_FNS[fn] on fresh leaves: -> (autograd's gradient tuple, radii)"""
    L = {k: v.detach().requires_grad_(True) for k, v in _params(s, fn, torch.float32, DEV).items()}
    m2 = torch.zeros_like(L["means3D"], requires_grad=True)
    c, r, d, a = HIP_FNS[fn](s.dcams[cam], L, m2, s.bg.to(DEV), s.deg)
    gl = torch.autograd.grad([c, d, a], [L[k] for k in NAMES] + [m2], _loss_grad(cam, c, d, a), allow_unused=True)
    return gl, r


def _pack_of(gl, r):
    return vp.pack_contribution(dict(zip(NAMES + ("means2D",), gl)), r)


def _equal_tuples(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_nested_request_keeps_the_outer_request_open():
    s = _scene("deg1")
    ref0, ref1 = _one_backward(s, cam=0), _one_backward(s, cam=1)
    with R.packed_gradients() as outer:
        with R.packed_gradients() as inner:
            g_in = _one_backward(s, cam=0)
            p_in = inner.take()
        g_out = _one_backward(s, cam=1)                # after the inner exit: still inside the outer request
        p_out = outer.take()
    assert p_in is not None and torch.equal(p_in, _pack_of(*ref0))
    assert p_out is not None and torch.equal(p_out, _pack_of(*ref1))
    assert _equal_tuples(g_in[0], ref0[0]) and _equal_tuples(g_out[0], ref1[0])
    # an inner request's pack belongs to the inner request: the outer one takes its own
    with R.packed_gradients() as outer:
        _one_backward(s, cam=1)
        with R.packed_gradients():
            _one_backward(s, cam=0)                    # (not taken)
        p_out = outer.take()
    assert p_out is not None and torch.equal(p_out, _pack_of(*ref1))
    assert R.packed_gradients.take() is None           # nothing left behind outside a request


@pytest.mark.parametrize("fn", ["twice", "precomp_and_default"])
def test_no_pack_when_more_than_one_rasterizer_backward_ran(fn):
    """Two rasterizer nodes in one autograd.grad under one request: no single pack holds the gradients, take() says so;
    autograd's gradients are the unpacked path's, bit for bit."""
    s = _scene("deg1")
    if fn == "twice":
        ref = _one_backward(s, "twice")
        with R.packed_gradients() as pg:
            got = _one_backward(s, "twice")
            pack = pg.take()
    else:                                              # an eligible node and an ineligible one, in one graph
        def both():
            L = {k: v.detach().requires_grad_(True) for k, v in _params(s, "default", torch.float32, DEV).items()}
            m2 = torch.zeros_like(L["means3D"], requires_grad=True)
            c1, r1, d1, a1 = HIP_FNS["default"](s.dcams[0], L, m2, s.bg.to(DEV), s.deg)
            c2, r2, d2, a2 = HIP_FNS["precomp"](s.dcams[0], L, m2, s.bg.to(DEV), s.deg)
            c, d, a = c1 + c2, d1 + d2, a1 + a2
            return torch.autograd.grad([c, d, a], [L[k] for k in NAMES] + [m2], _loss_grad(0, c, d, a)), r1
        ref = both()
        with R.packed_gradients() as pg:
            got = both()
            pack = pg.take()
    assert pack is None
    assert _equal_tuples(got[0], ref[0])


@pytest.mark.parametrize("bad", ["rows", "columns", "fp64", "host", "strided"])
def test_step_refuses_a_pack_that_does_not_fit_the_leaves(monkeypatch, bad):
    """A pack whose P or M (or dtype, device, layout) is not the leaves' is not used: the step packs autograd's result."""
    alter = {"rows": lambda p: p[:-1].contiguous(),
             "columns": lambda p: torch.cat([p, p[:, :3]], 1),
             "fp64": lambda p: p.double(),
             "host": lambda p: p.cpu(),
             "strided": lambda p: torch.cat([p, p], 1)[:, :p.shape[1]]}[bad]
    ref = _ref_a("deg1", "default")
    for name, n, kw, calls in MODES[:3]:
        log = _TakeLog(monkeypatch, alter)
        got = _run("deg1", "default", n, **kw)
        assert len(log.taken) == calls and all(p is not None for p in log.taken)
        _check_bits(got, _prefix(ref, n), (bad, name))
