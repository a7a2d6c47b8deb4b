"""Drop-in contract tests: the reference's call sites replayed against the HIP rasterizer.

* `render()`            gaussiansplatting/gaussian_renderer/__init__.py:18-104
* `Renderer.render()`   gs_renderer.py:923-1028
* the per-step access pattern of threestudio/systems/GaussianDreamer.py:234-306,378-408
  (8-view loop, radii max, viewspace_points.grad, densification statistic), and the
  no-grad validation path (GaussianDreamer.py:410-411).
The fake camera / model / pipe objects expose exactly the attributes the reference objects
have (scene/cameras.py:17-67, scene/gaussian_model.py:95-118, arguments/__init__.py:63-68).
"""
import math

import pytest
import torch

import oracle
from helpers import cov3d_from, make_scene, oracle_settings
from humangaussian_amd import synth
from humangaussian_amd.renderer import Renderer, render

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Pipe:
    convert_SHs_python = False
    compute_cov3D_python = False
    debug = False


class FakeCamera:
    """scene/cameras.py::Camera attribute surface (tensors on the device)."""

    def __init__(self, cam):
        self.image_height, self.image_width = cam.image_height, cam.image_width
        self.FoVx, self.FoVy = cam.FoVx, torch.tensor(cam.FoVy, device=DEV)   # FoVy arrives as a device tensor
        self.world_view_transform = cam.world_view_transform.to(DEV)
        self.full_proj_transform = cam.full_proj_transform.to(DEV)
        self.camera_center = cam.camera_center.to(DEV)


class FakeGaussianModel:
    """scene/gaussian_model.py::GaussianModel getters (activations included)."""

    def __init__(self, sc, sh_degree, max_sh_degree=None):
        self.active_sh_degree = sh_degree
        self.max_sh_degree = sh_degree if max_sh_degree is None else max_sh_degree
        p = lambda t: torch.nn.Parameter(t.to(DEV))  # noqa: E731
        self._xyz = p(sc["means3D"])
        self._features_dc = p(sc["shs"][:, :1].contiguous())
        self._features_rest = p(sc["shs"][:, 1:].contiguous())
        self._scaling = p(torch.log(sc["scales"]))
        self._rotation = p(sc["rotations"] * 1.7)                      # un-normalised, like training
        self._opacity = p(torch.logit(sc["opacities"].clamp(1e-4, 1 - 1e-4)))

    @property
    def get_xyz(self): return self._xyz
    @property
    def get_features(self): return torch.cat((self._features_dc, self._features_rest), dim=1)
    @property
    def get_opacity(self): return torch.sigmoid(self._opacity)
    @property
    def get_scaling(self): return torch.exp(self._scaling)
    @property
    def get_rotation(self): return torch.nn.functional.normalize(self._rotation)

    def get_covariance(self, scaling_modifier=1):
        sc = {"scales": self.get_scaling, "rotations": self.get_rotation}
        return cov3d_from(sc, scaling_modifier)

    def params(self):
        return [self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity]


def _scene(P=400, deg=1, **kw):
    sc = make_scene(P=P, sh_degree=deg, seed=17, H=64, W=80, spread=0.3, **kw)
    return sc, FakeGaussianModel(sc, deg), FakeCamera(sc["cam"])


def test_render_dict_contract_and_oracle_values():
    sc, pc, cam = _scene()
    bg = sc["bg"].to(DEV)
    out = render(cam, pc, Pipe(), bg)
    assert set(out) == {"render", "viewspace_points", "visibility_filter", "radii", "depth_3dgs", "alpha_3dgs"}
    assert out["render"].shape == (3, 64, 80) and out["depth_3dgs"].shape == (1, 64, 80)
    assert out["alpha_3dgs"].shape == (1, 64, 80) and out["radii"].dtype == torch.int32
    assert out["visibility_filter"].dtype == torch.bool and torch.equal(out["visibility_filter"], out["radii"] > 0)
    assert out["viewspace_points"].shape == pc.get_xyz.shape and out["viewspace_points"].requires_grad
    # zeros, like gaussian_renderer/__init__.py:26 (gaussiansplatting/train.py:113 -> gaussian_model.py:436 reads the VALUES)
    assert out["viewspace_points"].is_leaf and float(out["viewspace_points"].detach().abs().max()) == 0.0
    # values: the activated parameters through the oracle
    st = oracle_settings(sc)
    oc, orad, od, oa = oracle.rasterize(pc.get_xyz.detach().cpu(), None, pc.get_features.detach().cpu(), None,
                                        pc.get_opacity.detach().cpu(), pc.get_scaling.detach().cpu(),
                                        pc.get_rotation.detach().cpu(), None, st)
    assert torch.equal(out["radii"].cpu(), orad)
    assert float((out["render"].cpu() - oc).abs().max()) < 1e-4
    assert float((out["alpha_3dgs"].cpu() - oa).abs().max()) < 1e-4
    # gradients reach every raw parameter through the activations; means2D.grad is populated
    loss = out["render"].mean() + 0.1 * out["depth_3dgs"].mean()
    loss.backward()
    for p_ in pc.params():
        assert p_.grad is not None and torch.isfinite(p_.grad).all() and float(p_.grad.abs().max()) > 0
    g = out["viewspace_points"].grad
    assert g is not None and g.shape == (400, 3) and float(g[:, 2].abs().max()) == 0 and float(g[:, :2].abs().max()) > 0


def test_render_under_no_grad_and_amp_inputs():
    sc, pc, cam = _scene()
    bg = sc["bg"].to(DEV)
    ref = render(cam, pc, Pipe(), bg)
    with torch.no_grad():                                   # validation / test path
        out = render(cam, pc, Pipe(), bg)
    assert not out["render"].requires_grad and torch.equal(out["render"], ref["render"].detach())
    assert torch.equal(out["radii"], ref["radii"])
    with torch.autocast("cuda", dtype=torch.float16):       # Lightning 16-mixed: inputs are .float()'ed
        out16 = render(cam, pc, Pipe(), bg)
    assert out16["render"].dtype == torch.float32
    assert float((out16["render"] - ref["render"]).abs().max()) < 1e-4


def test_render_optional_branches_override_color_and_python_cov3d():
    sc, pc, cam = _scene(deg=0)
    bg = sc["bg"].to(DEV)
    ref = render(cam, pc, Pipe(), bg)
    pipe = Pipe(); pipe.compute_cov3D_python = True
    out = render(cam, pc, pipe, bg)
    assert torch.equal(out["radii"], ref["radii"]) and float((out["render"] - ref["render"]).abs().max()) < 2e-4
    colors = torch.rand(400, 3, device=DEV, requires_grad=True)
    out2 = render(cam, pc, Pipe(), bg, override_color=colors)
    out2["render"].sum().backward()
    assert colors.grad is not None and float(colors.grad.abs().max()) > 0
    pipe2 = Pipe(); pipe2.convert_SHs_python = True
    out3 = render(cam, pc, pipe2, bg)
    assert float((out3["render"] - ref["render"]).abs().max()) < 1e-4


def test_renderer_class_contract():
    sc, pc, cam = _scene()
    r = Renderer(pc, white_background=True, device=DEV)
    out = r.render(cam)
    assert set(out) == {"image", "depth", "alpha", "viewspace_points", "visibility_filter", "radii"}
    assert float(out["image"].min()) >= 0 and float(out["image"].max()) <= 1
    empty = out["alpha"][0] == 0
    assert bool(empty.any()) and float((out["image"][:, empty] - 1.0).abs().max()) == 0     # white background


def test_gaussiandreamer_step_access_pattern():
    """8-view loop + on_before_optimizer_step bookkeeping (GaussianDreamer.py:244-266,378-391)."""
    sc = make_scene(P=600, sh_degree=0, seed=23, H=64, W=64, spread=0.3)
    pc = FakeGaussianModel(sc, 0)
    bg = torch.zeros(3, device=DEV)
    cams = [FakeCamera(synth.orbit_camera(10.0 * (i % 3 - 1), 45.0 * i, 1.8, 50.0, 64, 64)) for i in range(8)]
    images, depths, viewspace_point_list, radii = [], [], [], None
    for i, cam in enumerate(cams):
        pkg = render(cam, pc, Pipe(), bg)
        viewspace_point_list.append(pkg["viewspace_points"])
        radii = pkg["radii"] if i == 0 else torch.max(pkg["radii"], radii)
        images.append(pkg["render"].permute(1, 2, 0)); depths.append(pkg["depth_3dgs"].permute(1, 2, 0))
    comp_rgb, depth = torch.stack(images, 0), torch.stack(depths, 0)
    opacity = depth / depth.max().detach()   # (the reference lets the max carry gradient; detached here
                                             #  so the loss splits exactly into per-view terms below)
    loss = ((comp_rgb - 0.5) ** 2).mean() + 0.1 * torch.sqrt(opacity ** 2 + 0.01).mean()
    loss.backward()
    viewspace_point_tensor_grad = torch.zeros_like(viewspace_point_list[0])
    for v in viewspace_point_list:
        assert v.grad is not None
        viewspace_point_tensor_grad = viewspace_point_tensor_grad + v.grad
    visibility_filter = radii > 0
    max_radii2D = torch.zeros(600, device=DEV)                                   # float, like the model's
    max_radii2D[visibility_filter] = torch.max(max_radii2D[visibility_filter], radii[visibility_filter])
    stat = torch.norm(viewspace_point_tensor_grad[visibility_filter, :2], dim=-1, keepdim=True)
    assert torch.isfinite(stat).all() and float(stat.max()) > 0 and int(visibility_filter.sum()) > 300
    # accumulated parameter gradients = sum of the per-view gradients (autograd accumulation)
    total = pc._xyz.grad.clone()
    pc._xyz.grad = None
    acc = torch.zeros_like(total)
    for i, cam in enumerate(cams):
        pkg = render(cam, pc, Pipe(), bg)
        # same loss restricted to view i (depth.max() is a global constant of the 8-view batch)
        li = ((pkg["render"].permute(1, 2, 0) - 0.5) ** 2).mean() / 8 + \
            0.1 * torch.sqrt((pkg["depth_3dgs"].permute(1, 2, 0) / depth.max().detach()) ** 2 + 0.01).mean() / 8
        g, = torch.autograd.grad(li, pc._xyz)
        acc += g
    assert float((acc - total).abs().max()) <= 2e-3 * float(total.abs().max())


@pytest.mark.gpu
def test_dist_cuda2_matches_kdtree_reference():
    """simple_knn._C.distCUDA2 replacement: mean squared distance to the 3 nearest neighbours
    (own index excluded, duplicates count) against a float64 k-d tree; call sites
    gaussian_model.py:134 / gs_renderer.py:386-389 clamp the result and take log(sqrt())."""
    import numpy as np
    from scipy.spatial import cKDTree
    from simple_knn._C import distCUDA2
    rng = np.random.default_rng(3)
    for n in (4, 257, 5000):
        pts = rng.normal(0, 0.4, (n, 3)).astype(np.float32)
        if n > 100:
            pts[10] = pts[11]                     # exact duplicates: distance 0 counts
            pts[20] = pts[21] = pts[22]
        d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4)
        ref = (d[:, 1:] ** 2).mean(1)
        got = distCUDA2(torch.from_numpy(pts).cuda()).cpu().numpy().astype(np.float64)
        assert got.shape == (n,)
        assert np.allclose(got, ref, rtol=2e-5, atol=1e-9), (n, np.abs(got - ref).max())
    assert distCUDA2(torch.zeros(0, 3).cuda()).shape == (0,)
    # the synthetic-cloud initialiser uses the same definition on the CPU
    from humangaussian_amd import synth
    pts = synth.humanoid_points(3000, seed=1)
    got = distCUDA2(torch.from_numpy(pts).cuda()).cpu().numpy()
    assert np.allclose(got, synth.mean_knn_dist2(pts), rtol=2e-5, atol=1e-9)


@pytest.mark.gpu
def test_dist_cuda2_grid_search_equals_the_brute_force_bit_for_bit():
    """The near-linear form (uniform grid + ring search, csrc/knn.hip; what upstream's Morton sort + box pruning is for,
    simple_knn.cu:63-221) returns the SAME three distances as the exact O(P^2) kernel on every kind of cloud: the avatar
    surface at the benchmark sizes, planar / collinear sets, duplicates, a box stretched by outliers, a cloud so
    degenerate (everything in one cell) that the device falls back to the brute force by itself."""
    import time
    import numpy as np
    from humangaussian_amd import synth
    from humangaussian_amd.knn import distCUDA2
    rng = np.random.default_rng(5)
    clouds = {
        "body_100k": synth.body_points(100_000, seed=0, source="capsule"),   # (pinned: the same cloud on every machine)
        "gauss": rng.normal(0, 0.4, (20_000, 3)),
        "planar": np.concatenate([rng.uniform(-1, 1, (5000, 2)), np.zeros((5000, 1))], 1),
        "collinear": np.stack([rng.uniform(-3, 3, 3000), np.zeros(3000), np.zeros(3000)], 1),
        "outliers": np.concatenate([rng.normal(0, 0.01, (6000, 3)), [[50.0, 0, 0], [-50.0, 0.3, 0]]]),
        "all_equal": np.full((6000, 3), 0.25),          # > 4096 points in one cell: the device picks the brute force
        "tiny": rng.normal(0, 1, (5, 3)),
        "two_scales": np.concatenate([rng.normal((0, 0, 0), 0.002, (4000, 3)), rng.normal((1, 1, 1), 0.3, (4000, 3))]),
        # translated far from the world origin: the ring search's stop rule works in grid-relative coordinates
        "translated_1e3": synth.body_points(30_000, seed=1, source="capsule") + np.float32(1.0e3),
        "translated_1e4": synth.body_points(30_000, seed=2, source="capsule") + np.array([1.0e4, -1.0e4, 3.0e3], np.float32),
    }
    dup = rng.normal(0, 0.2, (3000, 3))
    dup[5] = dup[6]
    dup[50] = dup[51] = dup[52] = dup[53]
    clouds["duplicates"] = dup
    for name, pts in clouds.items():
        p = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).cuda()
        grid, brute = distCUDA2(p), distCUDA2(p, brute_force=True)
        assert torch.equal(grid.view(torch.int32), brute.view(torch.int32)), (name, float((grid - brute).abs().max()))
    # configs[3]-sized cloud against the k-d tree, and the point of it: time
    pts = synth.body_points(500_000, seed=0, source="capsule")      # (the 20 ms bar was set on this cloud)
    p = torch.from_numpy(pts).cuda()
    distCUDA2(p)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = distCUDA2(p)
    torch.cuda.synchronize()
    t_grid = time.perf_counter() - t0
    assert np.allclose(got.cpu().numpy(), synth.mean_knn_dist2(pts), rtol=2e-5, atol=1e-12)
    print(f"KNN 500k points: grid {t_grid * 1e3:.2f} ms")
    assert t_grid < 0.02                                  # (the brute force takes ~60 ms here)


@pytest.mark.gpu
def test_dist_cuda2_grid_search_on_the_human_mesh_cloud():
    """The avatar surface sampled from the local human.obj asset (not shipped: built by humangaussian_amd/data): the grid
    search returns the brute force's distances bit for bit, and the k-d tree's values."""
    import numpy as np
    from humangaussian_amd import data, synth
    from humangaussian_amd.knn import distCUDA2
    if not data.have_human_mesh():
        pytest.skip("the local human.obj asset is missing (humangaussian_amd/data/make_human_mesh.py builds it)")
    for n, seed in ((100_000, 0), (30_000, 1)):
        pts = synth.body_points(n, seed=seed, source="human_obj")
        p = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).cuda()
        grid, brute = distCUDA2(p), distCUDA2(p, brute_force=True)
        assert torch.equal(grid.view(torch.int32), brute.view(torch.int32)), (n, float((grid - brute).abs().max()))
        assert np.allclose(grid.cpu().numpy(), synth.mean_knn_dist2(pts), rtol=2e-5, atol=1e-12), n


@pytest.mark.gpu
def test_view_pack_reduction_kernel_equals_rank_order_loop():
    """hgs_reduce_view_packs (what allgather_reduce runs on HIP tensors) against the rank-order
    torch loop the CPU/gloo tests exercise: sums bit-identical, radii column = max."""
    from humangaussian_amd import _lib
    g = torch.Generator().manual_seed(11)
    for world, P, F in ((1, 100, 18), (3, 1000, 18), (8, 4097, 63)):
        packs = torch.randn(world, P, F, generator=g)
        packs[:, :, -1] = torch.randint(0, 300, (world, P), generator=g).float()
        ref = packs[0].clone()
        for r in range(1, world):
            ref[:, :-1] += packs[r][:, :-1]
            ref[:, -1] = torch.maximum(ref[:, -1], packs[r][:, -1])
        got = _lib.load_binding().reduce_view_packs(packs.cuda()).cpu()
        assert torch.equal(got, ref), (world, P, F)


def test_debug_flag_path_gives_identical_results():
    """pipe.debug=True (gaussian_renderer/__init__.py:49): upstream's switch for surfacing device
    errors at the causing call; here it synchronises after each native call - same numbers."""
    import math
    from humangaussian_amd import GaussianRasterizationSettings, GaussianRasterizer
    sc = make_scene(P=400, sh_degree=1, seed=5, H=64, W=64)
    cam = sc["cam"]
    outs = []
    for dbg in (False, True):
        rs = GaussianRasterizationSettings(
            64, 64, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), sc["bg"].to(DEV), 1.0,
            cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), 1, cam.camera_center.to(DEV),
            False, dbg)
        ins = {k: sc[k].to(DEV).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        m2 = torch.zeros_like(ins["means3D"], requires_grad=True)
        c, r, d, a = GaussianRasterizer(rs)(means3D=ins["means3D"], means2D=m2, shs=ins["shs"],
                                            opacities=ins["opacities"], scales=ins["scales"],
                                            rotations=ins["rotations"])
        (c.sum() + d.sum() + a.sum()).backward()
        outs.append((c.detach(), r, ins["means3D"].grad, m2.grad))
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_view_pack_kernel_equals_torch_cat():
    from humangaussian_amd import view_parallel as vp
    g = torch.Generator().manual_seed(2)
    for P, M in ((1, 1), (777, 1), (300, 16)):
        grads = {"means3D": torch.randn(P, 3, generator=g), "means2D": torch.randn(P, 3, generator=g),
                 "shs": torch.randn(P, M, 3, generator=g), "opacities": torch.randn(P, 1, generator=g),
                 "scales": torch.randn(P, 3, generator=g), "rotations": torch.randn(P, 4, generator=g)}
        radii = torch.randint(0, 400, (P,), generator=g, dtype=torch.int32)
        ref = vp.pack_contribution(grads, radii)                          # CPU tensors: torch path
        got = vp.pack_contribution({k: v.cuda() for k, v in grads.items()}, radii.cuda()).cpu()
        assert got.shape == ref.shape and torch.equal(got, ref)
        back, r2 = vp.unpack_contribution(got, {k: v.shape for k, v in grads.items()})
        assert torch.equal(r2, radii) and all(torch.equal(back[k], grads[k]) for k in grads)


def test_mark_visible_matches_oracle_including_near_plane_boundary_and_empty():
    """`GaussianRasterizer.markVisible` / `hgs_mark_visible` (replaces `_C.mark_visible`): the frustum
    test is `view-space z > 0.2`, nothing else.  Checked against oracle.mark_visible on a cloud that
    straddles the camera, at the exact boundary (z == 0.2 is NOT visible, the next float is) and
    for P == 0, through the Python API and through the raw C ABI."""
    import ctypes
    import numpy as np
    from humangaussian_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib
    dev = torch.device("cuda")
    sc = make_scene(P=5000, sh_degree=0, seed=5, H=64, W=64, spread=2.5)     # many points behind the camera
    st = oracle_settings(sc)
    cam = sc["cam"]
    rs = GaussianRasterizationSettings(64, 64, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), sc["bg"].to(dev), 1.0,
                                       cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 0,
                                       cam.camera_center.to(dev), False, False)
    got = GaussianRasterizer(rs).markVisible(sc["means3D"].to(dev))
    ref = oracle.mark_visible(sc["means3D"], st)
    assert got.dtype == torch.bool and got.shape == (5000,)
    assert torch.equal(got.cpu(), ref) and 0 < int(ref.sum()) < 5000
    # exact boundary with an identity view matrix: view-space z == world z
    near = np.float32(0.2)
    zs = torch.tensor([float(near), float(np.nextafter(near, np.float32(1))), float(np.nextafter(near, np.float32(0))),
                       0.0, -1.0, 5.0], dtype=torch.float32)
    pts = torch.stack([torch.zeros(6), torch.zeros(6), zs], 1)
    rs_id = rs._replace(viewmatrix=torch.eye(4, device=dev), projmatrix=torch.eye(4, device=dev))
    got = GaussianRasterizer(rs_id).markVisible(pts.to(dev)).cpu()
    assert got.tolist() == [False, True, False, False, False, True]
    st_id = st._replace(viewmatrix=torch.eye(4), projmatrix=torch.eye(4))
    assert torch.equal(got, oracle.mark_visible(pts, st_id))
    # P == 0
    empty = GaussianRasterizer(rs).markVisible(torch.zeros(0, 3, device=dev))
    assert empty.shape == (0,) and empty.dtype == torch.bool
    # raw C ABI (include/hgs_rast.h: hgs_mark_visible), caller-owned buffers
    lib = _lib.load()
    s = _lib.HgsSettings()
    vm = cam.world_view_transform.to(dev).contiguous()
    s.image_height = s.image_width = 64
    s.viewmatrix = vm.data_ptr()
    m = sc["means3D"].to(dev).contiguous()
    present = torch.full((5000,), 7, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    rc = lib.hgs_mark_visible(ctypes.byref(s), 5000, ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(present.data_ptr()),
                              ctypes.c_void_p(stream.cuda_stream))
    stream.synchronize()
    assert rc == 0 and torch.equal(present.cpu().bool(), ref) and int(present.max()) == 1
    assert lib.hgs_mark_visible(ctypes.byref(s), 0, None, None, None) == 0


def test_convert_shs_python_branch_degree3_matches_rasterizer_sh():
    """pipe.convert_SHs_python (gaussian_renderer/__init__.py:73-78) at SH degree 3: colours computed
    in Python and handed over as colors_precomp give the image the in-kernel SH path gives."""
    dev = torch.device("cuda")
    sc = make_scene(P=400, sh_degree=3, seed=21, H=64, W=80, spread=0.3)
    pc = FakeGaussianModel(sc, 3)
    cam = FakeCamera(sc["cam"])

    class PyShPipe(Pipe):
        convert_SHs_python = True
    with torch.no_grad():
        a = render(cam, pc, PyShPipe(), sc["bg"].to(dev))
        b = render(cam, pc, Pipe(), sc["bg"].to(dev))
    assert float((a["render"] - b["render"]).abs().max()) < 2e-5
    assert torch.equal(a["radii"], b["radii"])


def test_reference_render_call_replayed_on_the_hip_rasterizer():
    """The arguments the reference's OWN render() (gaussian_renderer/__init__.py:18-104, run unchanged against the
    reference GaussianModel by tests/golden/make_render_call_fixture.py in the build container) hands to
    GaussianRasterizer.forward, replayed here through the HIP rasterizer and checked against the oracle:
    forward images <= 1e-4, radii exact, gradients <= 1e-3 max|g| (fp64 oracle)."""
    import os
    import numpy as np
    import oracle
    from humangaussian_amd import GaussianRasterizationSettings, GaussianRasterizer
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_render_call.npz"))
    H, W, tfx, tfy, mod, deg = fx["scalars"].tolist()
    H, W, deg = int(H), int(W), int(deg)
    dev = torch.device("cuda")
    t = lambda k: torch.from_numpy(fx[k].copy())  # noqa: E731
    rs = GaussianRasterizationSettings(H, W, tfx, tfy, t("bg").to(dev), mod, t("viewmatrix").to(dev), t("projmatrix").to(dev),
                                       deg, t("campos").to(dev), False, False)
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    ins = {k: t(k).to(dev).requires_grad_(True) for k in names}
    m2 = torch.zeros_like(ins["means3D"], requires_grad=True)
    c, r, d, a = GaussianRasterizer(rs)(means3D=ins["means3D"], means2D=m2, shs=ins["shs"], colors_precomp=None,
                                        opacities=ins["opacities"], scales=ins["scales"], rotations=ins["rotations"],
                                        cov3D_precomp=None)
    g = torch.Generator().manual_seed(4)
    wc, wd, wa = (torch.randn(s, generator=g) for s in ((3, H, W), (1, H, W), (1, H, W)))
    ((c * wc.to(dev)).sum() + (d * wd.to(dev)).sum() + (a * wa.to(dev)).sum()).backward()
    st = oracle.OracleSettings(H, W, tfx, tfy, t("bg"), mod, t("viewmatrix"), t("projmatrix"), deg, t("campos"), False, False)
    oin = {k: t(k).double().requires_grad_(True) for k in names}
    om2 = torch.zeros(oin["means3D"].shape, dtype=torch.float64, requires_grad=True)
    oc, orad, od, oa = oracle.rasterize(oin["means3D"], om2, oin["shs"], None, oin["opacities"], oin["scales"],
                                        oin["rotations"], None, st, dtype=torch.float64)
    ((oc * wc).sum() + (od * wd).sum() + (oa * wa).sum()).backward()
    assert torch.equal(r.cpu(), oracle.rasterize(t("means3D"), None, t("shs"), None, t("opacities"), t("scales"),
                                                 t("rotations"), None, st)[1])
    assert int((r > 0).sum()) > 300
    for got, ref in ((c, oc), (d, od), (a, oa)):
        assert float((got.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))
    for got, ref in [(ins[k].grad, oin[k].grad) for k in names] + [(m2.grad, om2.grad)]:
        assert float((got.cpu().double() - ref).abs().max()) <= 1e-3 * max(float(ref.abs().max()), 1e-12)


def test_backward_scratch_is_sized_by_the_published_pair_count():
    """The binding allocates the backward's pair rows per backward() call: by hgs_status.num_pairs of the forward call when
    the blend forward has published it (always the case once the device has been synchronised), else for the worst case
    of 16 pairs per entry.  Same gradients either way (tests/test_gpu_parity.py)."""
    from humangaussian_amd import _lib
    sc, pc, cam = _scene(P=2000, deg=0)
    bg = torch.zeros(3, device=DEV)
    out = render(cam, pc, Pipe(), bg)
    torch.cuda.synchronize()
    (out["render"].sum() + out["depth_3dgs"].sum()).backward()
    torch.cuda.synchronize()
    st = _lib.load_binding().device_state(0)
    R, pairs = int(st["max_R"]), int(st["bwd_pairs_last"])
    assert 0 < pairs <= 16 * R
    assert int(st["bwd_scratch_last"]) == -(-(R * 48 + pairs * 40) // 256) * 256 < -(-(R * 688) // 256) * 256
    assert all(torch.isfinite(p.grad).all() for p in pc.params() if p.grad is not None)
