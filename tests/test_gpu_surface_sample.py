"""GPU tests of the surface sampler and of the initial Gaussians (csrc/surface.hip through humangaussian_amd.surface).

Samples: the kernel is held to the numpy restatement (tests/surface_sample_reference.py) EXACTLY - face, uvw and the fp32
points bit for bit, for every sample of every case; test_surface_sample_cpu.py shows that no sample of these cases lies near
enough to a table boundary for the two summation orders to disagree.  Against the fp64 point the project's gate applies: error
<= 4 x the fp32 restatement's own error, floor 16 eps32 max|v| (the restatement's own error measured 0.8 eps32 max|v|).
HGS_WRITE_PROFILES=1 records the ratios in profiles/surface_sample_parity.json.

create_from_points: `rotation`, `max_radii2D`, `features_rest` and `opacity` are exact; `scaling` and `features_dc` are
measured against the fp64 formulas on the kernel's own distCUDA2 output, gate 4 x the error of the reference's torch chain
on the device, floor 4 eps32 |value|.  The clouds are uniform in [0, 0.3]^3: every finite mean squared distance is then
below 0.27 (the lone point of P = 1 has none: +inf, which both sides must pass on), so |scaling| = |ln(d) / 2| > 0.65 and the floor (4 x 2^-23 |value|) stays above what one correctly rounded square
root (2^-24 absolute in the logarithm) and a logarithm good to an ulp can add up to; nearer to d = 1 the value goes
through 0 and a relative floor would mean nothing."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import surface_sample_reference as ref
from humangaussian_amd import surface

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
EPS32 = 2.0 ** -23
CASES = ref.cases()
_BY_NAME = {c[0]: c for c in CASES}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def _mesh(F, variant):
    return ref.soup(F, variant)


@functools.lru_cache(maxsize=None)
def _expected(name):
    _, F, variant, N = _BY_NAME[name]
    v, f = _mesh(F, variant)
    return ref.sample(v, f, N, seed=ref.SAMPLE_SEED)


@functools.lru_cache(maxsize=None)
def _sampler(F, variant):
    v, f = _mesh(F, variant)
    return surface.SurfaceSampler(v, f)


_RATIOS = {}


def _record(name, entry):
    _RATIOS[name] = entry
    if os.environ.get("HGS_WRITE_PROFILES"):
        doc = {"what": "per case of tests/test_gpu_surface_sample.py: largest |point - fp64 point| of hgs_surface_sample and of "
                       "the fp32 numpy restatement, in units of eps32 max|v|, and the gate (4 x the second, at least 16) the "
                       "first is held to",
               "device": torch.cuda.get_device_name(0), "cases": dict(sorted(_RATIOS.items()))}
        with open(os.path.join(ROOT, "profiles", "surface_sample_parity.json"), "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_samples_equal_the_restatement(name):
    _, F, variant, N = _BY_NAME[name]
    v, f = _mesh(F, variant)
    want = _expected(name)
    s = _sampler(F, variant)
    pts, face, uvw = s.sample(N, seed=ref.SAMPLE_SEED, return_anchors=True)
    assert pts.shape == (N, 3) and face.shape == (N,) and uvw.shape == (N, 3)
    assert pts.dtype == uvw.dtype == torch.float32 and face.dtype == torch.int32
    # 5, 6: the table
    assert s.num_faces == F and s.num_sampled_faces == want["num_positive"]
    cdf = s.cdf.cpu().numpy()
    assert cdf.shape == (F,) and cdf.dtype == np.float64 and (np.diff(cdf) >= 0).all() and cdf[0] >= 0
    assert abs(cdf[-1] - want["cdf"][-1]) <= F * 2.0 ** -52 * want["cdf"][-1]
    assert s.area == cdf[-1]
    if N == 0:
        assert s.sample(0).shape == (0, 3)
        return
    p, fa, w = pts.cpu().numpy(), face.cpu().numpy(), uvw.cpu().numpy()
    # 1: face and uvw of every sample
    assert np.array_equal(fa, want["face"]), (name, int((fa != want["face"]).sum()))
    assert np.array_equal(_bits(w), _bits(want["uvw"]))
    # 2: the points, bit for bit; and as anchors on the same mesh
    assert np.array_equal(_bits(p), _bits(want["points"]))
    again = s.anchors(face, uvw).positions(s.vertices).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(p))
    # 3: against the fp64 point
    unit = EPS32 * float(np.abs(v[np.isfinite(v)]).max())
    e_hip = float(np.abs(p.astype(np.float64) - want["points64"]).max()) / unit
    e_ref = float(np.abs(want["points"].astype(np.float64) - want["points64"]).max()) / unit
    entry = {"hip_err": e_hip, "fp32_restatement_err": e_ref, "gate": max(4 * e_ref, 16.0)}
    print(name, entry)
    _record(name, entry)
    assert np.isfinite(p).all() and e_hip <= entry["gate"], (name, entry)
    # 4: the same bits again; an offset call is a slice of the larger one; points alone are the same points
    p2, f2, w2 = s.sample(N, seed=ref.SAMPLE_SEED, return_anchors=True)
    assert torch.equal(p2, pts) and torch.equal(f2, face) and torch.equal(w2, uvw)
    assert torch.equal(s.sample(N, seed=ref.SAMPLE_SEED), pts)
    k, m = N // 3, N - N // 3 - N // 4
    p3, f3, w3 = s.sample(m, seed=ref.SAMPLE_SEED, offset=k, return_anchors=True)
    assert torch.equal(p3, pts[k:k + m]) and torch.equal(f3, face[k:k + m]) and torch.equal(w3, uvw[k:k + m])


def test_seed_and_offset_use_all_64_bits():
    s = _sampler(65, "plain")
    v, f = _mesh(65, "plain")
    seed, offset = (0xdeadbeef << 32) | 0x12345678, (1 << 32) - 100
    want = ref.sample(v, f, 300, seed=seed, offset=offset)
    if want["margin"].min() <= ref.honest_margin(65):
        pytest.fail("the case is not honest: choose another seed")
    pts, face, uvw = s.sample(300, seed=seed, offset=offset, return_anchors=True)
    assert np.array_equal(face.cpu().numpy(), want["face"]) and np.array_equal(_bits(uvw.cpu().numpy()), _bits(want["uvw"]))
    assert np.array_equal(_bits(pts.cpu().numpy()), _bits(want["points"]))


def test_sample_surface_and_device_tensors():
    v, f = _mesh(65, "plain")
    want = ref.sample(v, f, 257, seed=0)
    pts, face = surface.sample_surface(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV), 257)
    assert face.dtype == torch.int64 and np.array_equal(face.cpu().numpy(), want["face"])
    assert np.array_equal(_bits(pts.cpu().numpy()), _bits(want["points"]))


def test_a_mesh_without_area_is_refused():
    v = np.zeros((6, 3), np.float32)
    with pytest.raises(ValueError, match="positive area"):
        surface.SurfaceSampler(v, np.arange(6, dtype=np.int32).reshape(2, 3))


# ---- create_from_points / create_from_pcd ---------------------------------------------------------------------------------

OPACITY = np.float32(np.log(np.float64(np.float32(0.1) / (np.float32(1.0) - np.float32(0.1)))))
C0 = 0.28209479177387814


@functools.lru_cache(maxsize=None)
def _cloud(P):
    rng = np.random.default_rng(500 + P)
    return (rng.uniform(0.0, 0.3, (P, 3)).astype(np.float32), rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32))


def _gate(name, got, torch_chain, want64):
    """|got - want64| <= max(4 x the torch chain's largest error, 4 eps32 |want64|), elementwise; non-finite values must agree"""
    fin = np.isfinite(want64)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin].astype(np.float64), want64[~fin], equal_nan=True)
    e_got = np.abs(got.astype(np.float64)[fin] - want64[fin])
    e_torch = np.abs(torch_chain.astype(np.float64)[fin] - want64[fin])
    gate = np.maximum(4 * (e_torch.max() if e_torch.size else 0.0), 4 * EPS32 * np.abs(want64[fin]))
    print(name, "max err", e_got.max() if e_got.size else 0.0, "torch chain", e_torch.max() if e_torch.size else 0.0)
    assert (e_got <= gate).all(), (name, float(e_got.max()), float(gate.min()))


@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("degree", [0, 1, 3])
@pytest.mark.parametrize("P", [1, 4, 255, 256, 257])
def test_create_from_points(P, degree, with_colors):
    from humangaussian_amd.knn import distCUDA2
    M = (degree + 1) ** 2
    pts_np, col_np = _cloud(P)
    pts = torch.as_tensor(pts_np, device=DEV)
    col = torch.as_tensor(col_np, device=DEV) if with_colors else None
    t = surface.create_from_points(pts, col, max_sh_degree=degree)
    shapes = {"xyz": (P, 3), "features_dc": (P, 1, 3), "features_rest": (P, M - 1, 3), "scaling": (P, 3), "rotation": (P, 4),
              "opacity": (P, 1), "max_radii2D": (P,)}
    assert set(t) == set(shapes)
    for k, shp in shapes.items():
        assert tuple(t[k].shape) == shp and t[k].dtype == torch.float32 and t[k].is_contiguous() and t[k].is_cuda, k
    assert torch.equal(t["xyz"], pts)
    # exact outputs
    assert np.array_equal(t["rotation"].cpu().numpy(), np.tile(np.array([1, 0, 0, 0], np.float32), (P, 1)))
    assert not t["max_radii2D"].any() and not t["features_rest"].any()
    assert np.array_equal(_bits(t["opacity"].cpu().numpy()), _bits(np.full((P, 1), OPACITY, np.float32)))
    # scaling and features_dc against fp64, on the kernel's own distCUDA2 output
    d = distCUDA2(pts)
    d64 = d.cpu().numpy().astype(np.float64)
    with np.errstate(all="ignore"):
        s64 = np.log(np.sqrt(np.where(d64 < np.float64(np.float32(1e-7)), np.float64(np.float32(1e-7)), d64)))
    s_torch = torch.log(torch.sqrt(torch.clamp_min(d, 0.0000001)))[..., None].repeat(1, 3)
    _gate("scaling", t["scaling"].cpu().numpy(), s_torch.cpu().numpy(), np.repeat(s64[:, None], 3, 1))
    c32 = col_np if with_colors else np.full((P, 3), 0.5, np.float32)
    dc64 = (c32.astype(np.float64) - 0.5) / C0
    dc_torch = (torch.as_tensor(c32, device=DEV) - 0.5) / C0                    # RGB2SH (utils/sh_utils.py)
    _gate("features_dc", t["features_dc"].cpu().numpy().reshape(P, 3), dc_torch.cpu().numpy(), dc64)
    if not with_colors:
        assert not t["features_dc"].any()


class _Model:
    """The reference GaussianModel's attributes and getters (gaussian_model.py:47-115) with nothing set yet"""

    def __init__(self, degree):
        self.active_sh_degree, self.max_sh_degree = 0, degree

    get_xyz = property(lambda m: m._xyz)
    get_features = property(lambda m: torch.cat((m._features_dc, m._features_rest), dim=1))
    get_opacity = property(lambda m: torch.sigmoid(m._opacity))
    get_scaling = property(lambda m: torch.exp(m._scaling))
    get_rotation = property(lambda m: torch.nn.functional.normalize(m._rotation))


class _Pcd:
    def __init__(self, points, colors):
        self.points, self.colors = points, colors


@pytest.mark.parametrize("source", ["pcd", "tensor"])
def test_create_from_pcd_sets_the_reference_parameters(source):
    P, degree = 257, 3
    pts_np, col_np = _cloud(P)
    model = _Model(degree)
    if source == "pcd":
        out = surface.create_from_pcd(model, _Pcd(pts_np.astype(np.float64), col_np.astype(np.float64)), 2.5)
        want = surface.create_from_points(torch.as_tensor(pts_np, device=DEV), torch.as_tensor(col_np, device=DEV), degree)
    else:
        given = torch.as_tensor(pts_np, device=DEV)
        out = surface.create_from_pcd(model, given, 2.5)
        want = surface.create_from_points(given, None, degree)
        assert model._xyz.data_ptr() != given.data_ptr()                         # the model owns its points
    assert out is model and model.spatial_lr_scale == 2.5
    shapes = {"_xyz": (P, 3), "_features_dc": (P, 1, 3), "_features_rest": (P, 15, 3), "_scaling": (P, 3),
              "_rotation": (P, 4), "_opacity": (P, 1)}
    for k, shp in shapes.items():
        p = getattr(model, k)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.is_contiguous(), k
        assert tuple(p.shape) == shp and p.dtype == torch.float32 and p.is_cuda, k
        assert torch.equal(p.detach(), want[k[1:]]), k
    assert not isinstance(model.max_radii2D, torch.nn.Parameter) and not model.max_radii2D.requires_grad
    assert tuple(model.max_radii2D.shape) == (P,) and model.max_radii2D.is_cuda and not model.max_radii2D.any()


# ---- end to end -------------------------------------------------------------------------------------------------------------

def test_init_from_body_renders_and_stays_anchored():
    from humangaussian_amd import synth
    from humangaussian_amd.renderer import cameras_from_c2w, render
    v, f = synth.humanoid_mesh()
    model = _Model(0)
    anchors = surface.init_from_body(model, v, f, 2000, seed=3)
    assert tuple(model._xyz.shape) == (2000, 3) and anchors.mapping_face.shape == (2000,)
    cam = cameras_from_c2w(synth.c2w_orbit(0.0, 90.0, 2.5)[None], math.radians(50.0), 64, 64, device=DEV)[0]
    with torch.no_grad():
        out = render(cam, model, None, torch.ones(3, device=DEV))
    assert out["render"].shape == (3, 64, 64) and bool(torch.isfinite(out["render"]).all())
    assert float(out["alpha_3dgs"].max()) > 0.0 and int((out["radii"] > 0).sum()) > 0
    # born anchored: the rest mesh gives the cloud back bit for bit; a translated mesh carries it along
    rest = torch.as_tensor(v, device=DEV)
    assert torch.equal(anchors.positions(rest), model._xyz.detach())
    shift = torch.tensor([0.25, -0.5, 0.125], device=DEV)
    moved = anchors.positions(rest + shift)
    bound = 4 * EPS32 * float((rest + shift).abs().max())
    assert float((moved - (model._xyz.detach() + shift)).abs().max()) <= bound
