"""The reference's OWN `render()` at this repo's rasterizer boundary (no GPU needed), replayed from
tests/golden/reference_import_calls.npz.  tests/golden/make_reference_import_fixture.py recorded it where the reference
tree exists, by importing the reference modules unchanged with this repo's `diff_gaussian_rasterization/` and
`simple_knn/` shims on sys.path:

  gaussiansplatting/gaussian_renderer/__init__.py:14   from diff_gaussian_rasterization import ...
  gaussiansplatting/scene/gaussian_model.py:20         from simple_knn._C import distCUDA2

and running the real `render()` (gaussian_renderer/__init__.py:18-104) against the real `GaussianModel` getters.  Here
the recorded imports must still resolve to this repo's objects, the recorded settings construction and rasterizer call
(`:86-94`) must still bind to `GaussianRasterizationSettings` and `GaussianRasterizer.forward` and carry exactly the
tensors our forward expects, and humangaussian_amd.renderer.render must hand the rasterizer the same arguments.
"""
import importlib
import importlib.util
import inspect
import json
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_reference_import_fixture",
                                                  os.path.join(GOLD, "make_reference_import_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def record():
    z = np.load(os.path.join(GOLD, "reference_import_calls.npz"))
    meta = json.loads(str(z["meta"]))
    arrays = {k: torch.from_numpy(z[k].copy()) for k in z.files if k != "meta"}
    return meta, arrays


def _resolve(qualname):
    mod, _, name = qualname.rpartition(".")
    return getattr(importlib.import_module(mod), name)


def _settings_kwargs(meta, arrays, call):
    """The keywords the reference constructed GaussianRasterizationSettings with, and their recorded values."""
    c = meta["calls"][call]
    vals = dict(c["settings"], **{f: arrays[f"{call}.settings.{f}"] for f in _generator().SETTINGS_TENSORS})
    assert c["settings_call"]["nargs"] == 0 and sorted(vals) == c["settings_call"]["kwargs"]
    return vals


def test_reference_render_binds_to_our_rasterizer(record):
    meta, arrays = record
    import diff_gaussian_rasterization as dgr
    from humangaussian_amd import rasterizer as ours
    from simple_knn._C import distCUDA2
    from humangaussian_amd.knn import distCUDA2 as our_knn
    # the names the reference imported ARE this repo's objects, and the shims still provide them
    assert dgr.GaussianRasterizer is ours.GaussianRasterizer and dgr.GaussianRasterizationSettings is ours.GaussianRasterizationSettings
    assert distCUDA2 is our_knn
    assert sorted(meta["imports"]) == ["gaussiansplatting.gaussian_renderer.GaussianRasterizationSettings",
                                       "gaussiansplatting.gaussian_renderer.GaussianRasterizer",
                                       "gaussiansplatting.scene.gaussian_model.distCUDA2"]
    for ref_name, imp in meta["imports"].items():
        name = ref_name.rpartition(".")[2]
        assert getattr(importlib.import_module(imp["from"]), name) is _resolve(imp["is"]), ref_name
    assert _resolve(meta["imports"]["gaussiansplatting.gaussian_renderer.GaussianRasterizer"]["is"]) is ours.GaussianRasterizer

    c = meta["calls"]["bind"]
    P, deg = 7, 1
    # the settings the reference built: our class, built with the reference's keywords, holds the recorded values
    assert c["settings_type"] == f"{ours.GaussianRasterizationSettings.__module__}.{ours.GaussianRasterizationSettings.__qualname__}"
    s = ours.GaussianRasterizationSettings(**_settings_kwargs(meta, arrays, "bind"))
    assert (s.image_height, s.image_width, s.sh_degree, s.prefiltered, s.debug) == (32, 48, 1, False, False)
    assert abs(s.tanfovx - 0.4830550656) < 1e-6 and s.scale_modifier == 1.0
    # the reference's rasterizer call, bound exactly as Python binds it to OUR forward
    fc = c["forward_call"]
    assert fc["nargs"] == 0
    kwargs = {k: (None if k in fc["none"] else arrays[f"bind.arg.{k}"]) for k in fc["kwargs"]}
    ba = inspect.signature(ours.GaussianRasterizer.forward).bind(ours.GaussianRasterizer(s), **kwargs)
    ba.apply_defaults()
    seen = ba.arguments
    # what arrived at the boundary (gaussian_renderer/__init__.py:86-94)
    assert seen["means3D"].shape == (P, 3) and seen["means2D"].shape == (P, 3) and c["requires_grad"]["means2D"]
    assert seen["shs"].shape == (P, (deg + 1) ** 2, 3) and seen["colors_precomp"] is None
    assert seen["opacities"].shape == (P, 1) and float(seen["opacities"].min()) > 0       # sigmoid applied
    assert seen["scales"].shape == (P, 3) and float(seen["scales"].min()) > 0             # exp applied
    assert torch.allclose(seen["rotations"].norm(dim=1), torch.ones(P))                   # normalised
    assert seen["cov3D_precomp"] is None
    assert set(c["out_keys"]) == {"render", "viewspace_points", "visibility_filter", "radii", "depth_3dgs", "alpha_3dgs"}
    assert c["visibility_filter_dtype"] == str(torch.bool)


def test_our_render_mirror_matches_reference_render_arguments(record, monkeypatch):
    """humangaussian_amd.renderer.render hands the rasterizer the same arguments as the
    reference's render() for the same camera / model / pipe."""
    meta, arrays = record
    from humangaussian_amd import rasterizer as ours
    from humangaussian_amd import renderer as mirror
    gen = _generator()
    c, rec = gen.CALLS["mirror"], meta["calls"]["mirror"]

    class Model:            # the reference GaussianModel's getters, returning what they returned for the recorded call
        active_sh_degree = rec["active_sh_degree"]
    pc = Model()
    for k in gen.GETTERS:
        setattr(pc, k, arrays[f"mirror.{k}"])
    cam = types.SimpleNamespace(FoVx=c["fovx"], FoVy=c["fovy"], image_height=c["H"], image_width=c["W"],
                                world_view_transform=torch.eye(4) * c["view"], full_proj_transform=torch.eye(4) * c["proj"],
                                camera_center=torch.ones(3) * c["campos"])
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    calls = []
    real_sig = inspect.signature(ours.GaussianRasterizer.forward)

    def fake_forward(self, *args, **kwargs):
        ba = real_sig.bind(self, *args, **kwargs)
        ba.apply_defaults()
        calls.append((dict(ba.arguments), self.raster_settings))
        n = ba.arguments["means3D"].shape[0]
        H, W = self.raster_settings.image_height, self.raster_settings.image_width
        return torch.zeros(3, H, W), torch.ones(n, dtype=torch.int32), torch.zeros(1, H, W), torch.zeros(1, H, W)

    monkeypatch.setattr(ours.GaussianRasterizer, "forward", fake_forward)
    b = mirror.render(cam, pc, pipe, torch.tensor(c["bg"]), c["mod"])
    (kb, sb), = calls
    assert sorted(b) == rec["out_keys"]
    for k in ("means3D", "shs", "opacities", "scales", "rotations"):
        assert torch.equal(kb[k], arrays[f"mirror.arg.{k}"]), k
    assert kb["means2D"].shape == arrays["mirror.arg.means2D"].shape and kb["means2D"].requires_grad
    assert sorted(k for k, v in kb.items() if v is None) == rec["forward_call"]["none"] == ["colors_precomp", "cov3D_precomp"]
    for f in ("image_height", "image_width", "tanfovx", "tanfovy", "scale_modifier", "sh_degree", "prefiltered", "debug"):
        assert getattr(sb, f) == rec["settings"][f], f
    for f in ("bg", "viewmatrix", "projmatrix", "campos"):
        assert torch.equal(getattr(sb, f), arrays[f"mirror.settings.{f}"]), f
