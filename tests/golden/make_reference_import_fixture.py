"""Generates tests/golden/reference_import_calls.npz: what the reference's OWN `render()`
(gaussiansplatting/gaussian_renderer/__init__.py:18-104), imported unchanged with this repo's `diff_gaussian_rasterization/`
and `simple_knn/` shims on sys.path, does at the rasterizer boundary for two small reference `GaussianModel`s:

  imports   which of this repo's objects the reference modules bound, and the shim module each came from
  per call  the keywords it constructs GaussianRasterizationSettings with and the settings' values, the arguments it hands
            GaussianRasterizer.forward (call form and tensors), the getter outputs of the model, the keys of its result

Run where the reference tree exists (it imports the reference; nothing else does):

    python tests/golden/make_reference_import_fixture.py [REFERENCE_ROOT]

tests/test_reference_import_cpu.py replays the record against the shims, the current forward signature and
humangaussian_amd.renderer.render."""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "reference_import_calls.npz")
SETTINGS_TENSORS = ("bg", "viewmatrix", "projmatrix", "campos")
SETTINGS_SCALARS = ("image_height", "image_width", "tanfovx", "tanfovy", "scale_modifier", "sh_degree", "prefiltered", "debug")
GETTERS = ("get_xyz", "get_features", "get_opacity", "get_scaling", "get_rotation")
# the two calls of tests/test_reference_import_cpu.py: model size / SH degree / seed, camera, bg, scaling modifier
CALLS = {
    "bind": dict(P=7, deg=1, seed=0, grad=True, H=32, W=48, fovx=0.9, fovy=0.8, view=1.0, proj=1.0, campos=0.0,
                 bg=(0.0, 0.0, 0.0), mod=None),
    "mirror": dict(P=5, deg=2, seed=1, grad=False, H=16, W=16, fovx=1.1, fovy=0.7, view=2.0, proj=3.0, campos=1.0,
                   bg=(0.1, 0.2, 0.3), mod=0.7),
}


def _import_reference(ref):
    sys.path[:0] = [ref, ROOT]
    ply = types.ModuleType("plyfile")                 # `plyfile` is not needed: the model only needs the names at import time
    ply.PlyData = ply.PlyElement = object
    sys.modules["plyfile"] = ply
    scene = types.ModuleType("gaussiansplatting.scene")   # register the package without its COLMAP readers (PIL, ...)
    scene.__path__ = [os.path.join(ref, "gaussiansplatting", "scene")]
    sys.modules["gaussiansplatting.scene"] = scene
    import gaussiansplatting.gaussian_renderer as gr
    import gaussiansplatting.scene.gaussian_model as gm
    return gr, gm


def _qualname(obj):
    return f"{obj.__module__}.{obj.__qualname__}"


def main(ref):
    gr, gm = _import_reference(ref)
    import diff_gaussian_rasterization
    import simple_knn._C
    from humangaussian_amd import rasterizer as ours
    shims = (diff_gaussian_rasterization, simple_knn._C)
    imports = {}
    for mod, names in ((gr, ("GaussianRasterizer", "GaussianRasterizationSettings")), (gm, ("distCUDA2",))):
        for name in names:
            obj = getattr(mod, name)
            src = [m.__name__ for m in shims if getattr(m, name, None) is obj]
            assert len(src) == 1, (mod.__name__, name)
            imports[f"{mod.__name__}.{name}"] = {"from": src[0], "is": _qualname(obj)}

    _zl = torch.zeros_like                            # render() hard-codes device="cuda" (gaussian_renderer/__init__.py:26)
    torch.zeros_like = lambda t, **k: _zl(t, **{**k, "device": "cpu"}) if "device" in k else _zl(t, **k)
    real_settings, real_forward = gr.GaussianRasterizationSettings, ours.GaussianRasterizer.forward
    sig = inspect.signature(real_forward)
    arrays, calls = {}, {}
    for name, c in CALLS.items():
        P, deg = c["P"], c["deg"]
        pc = gm.GaussianModel(deg)
        g = torch.Generator().manual_seed(c["seed"])
        pc._xyz = torch.randn(P, 3, generator=g)
        pc._features_dc = torch.randn(P, 1, 3, generator=g)
        pc._features_rest = torch.randn(P, (deg + 1) ** 2 - 1, 3, generator=g)
        pc._scaling = torch.randn(P, 3, generator=g)
        pc._rotation = torch.randn(P, 4, generator=g)
        pc._opacity = torch.randn(P, 1, generator=g)
        for k in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
            getattr(pc, k).requires_grad_(c["grad"])
        pc.active_sh_degree = deg
        cam = types.SimpleNamespace(FoVx=c["fovx"], FoVy=c["fovy"], image_height=c["H"], image_width=c["W"],
                                    world_view_transform=torch.eye(4) * c["view"], full_proj_transform=torch.eye(4) * c["proj"],
                                    camera_center=torch.ones(3) * c["campos"])
        pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
        seen = {}

        def settings(*args, **kwargs):
            seen["settings_call"] = {"nargs": len(args), "kwargs": sorted(kwargs)}
            return real_settings(*args, **kwargs)

        def fake_forward(self, *args, **kwargs):
            ba = sig.bind(self, *args, **kwargs)
            ba.apply_defaults()
            seen["forward_call"] = {"nargs": len(args), "kwargs": sorted(kwargs),
                                    "none": sorted(k for k, v in ba.arguments.items() if v is None)}
            seen["args"] = {k: v for k, v in ba.arguments.items() if isinstance(v, torch.Tensor)}
            seen["settings"] = self.raster_settings
            H, W = self.raster_settings.image_height, self.raster_settings.image_width
            n = ba.arguments["means3D"].shape[0]
            return torch.zeros(3, H, W), torch.ones(n, dtype=torch.int32), torch.zeros(1, H, W), torch.zeros(1, H, W)

        gr.GaussianRasterizationSettings, ours.GaussianRasterizer.forward = settings, fake_forward
        try:
            bg = torch.tensor(c["bg"])
            out = gr.render(cam, pc, pipe, bg) if c["mod"] is None else gr.render(cam, pc, pipe, bg, c["mod"])
        finally:
            gr.GaussianRasterizationSettings, ours.GaussianRasterizer.forward = real_settings, real_forward
        s = seen["settings"]
        calls[name] = {
            "forward_call": seen["forward_call"], "settings_call": seen["settings_call"],
            "settings_type": _qualname(type(s)),
            "settings": {f: getattr(s, f) for f in SETTINGS_SCALARS},
            "requires_grad": {k: bool(v.requires_grad) for k, v in seen["args"].items()},
            "out_keys": sorted(out), "visibility_filter_dtype": str(out["visibility_filter"].dtype),
            "active_sh_degree": pc.active_sh_degree,
        }
        for k, v in seen["args"].items():
            arrays[f"{name}.arg.{k}"] = v.detach().numpy()
        for f in SETTINGS_TENSORS:
            arrays[f"{name}.settings.{f}"] = getattr(s, f).detach().numpy()
        for k in GETTERS:
            arrays[f"{name}.{k}"] = getattr(pc, k).detach().numpy()
    torch.zeros_like = _zl
    np.savez_compressed(OUT, meta=np.array(json.dumps({"imports": imports, "calls": calls}, sort_keys=True)), **arrays)
    print("wrote", OUT, sorted(arrays))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
