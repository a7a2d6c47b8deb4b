"""Generates tests/golden/reference_fields.npz: the reference's own `GaussianModel.extract_fields`
(/root/reference/gs_renderer.py:240-331) run on the CPU on a small cloud - the inputs, the field, `center` and `scale`.
Run in the build container (imports /root/reference, which does not exist on the GPU box):

    python tests/golden/make_fields_fixture.py

The modules the reference imports at the top of gs_renderer.py and does not need for this (plyfile, kiui) are stubbed.
The cloud: 3000 Gaussians on a 0.25 x 0.15 x 0.75 ellipsoid, scales 0.02 exp(0.6 N), random quaternions, opacities
0.002 + 0.95 U (some below the 0.005 cut), resolution 32, 8 blocks per axis.  `meta` also stores how far the fp64
restatement (tests/fields_reference.py) is from the recording: the yardstick of the GPU test."""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REF, ROOT, os.path.join(ROOT, "tests")]
for name, attrs in (("plyfile", ("PlyData", "PlyElement")), ("kiui", ()), ("kiui.sh", ("eval_sh", "SH2RGB", "RGB2SH")),
                    ("kiui.mesh", ("Mesh",)), ("kiui.mesh_utils", ("decimate_mesh", "clean_mesh"))):
    mod = types.ModuleType(name)
    for a in attrs:
        setattr(mod, a, object)
    sys.modules[name] = mod
sys.modules["kiui"].lo = lambda *a, **k: None
_zeros = torch.zeros
torch.zeros = lambda *a, **k: _zeros(*a, **{**k, "device": "cpu"}) if "device" in k else _zeros(*a, **k)

import gs_renderer  # noqa: E402
import fields_reference as FR  # noqa: E402

N, RES, NB, SEED = 3000, 32, 8, 3
xyz, opacity, scaling, rotation = FR.cloud(N, SEED)
pc = gs_renderer.GaussianModel(0)
pc._xyz = torch.from_numpy(xyz)
pc._scaling = torch.log(torch.from_numpy(scaling))                 # raw: get_scaling = exp
pc._rotation = torch.from_numpy(rotation)
pc._opacity = gs_renderer.inverse_sigmoid(torch.from_numpy(opacity))   # raw: get_opacity = sigmoid
with torch.no_grad():
    occ = pc.extract_fields(resolution=RES, num_blocks=NB).numpy()
    # what the model hands to the field: the activations of the raw parameters (not bit-equal to the arrays above)
    ins = dict(xyz=pc.get_xyz.numpy(), opacity=pc.get_opacity.numpy(), scaling=pc.get_scaling.numpy(),
               rotation=pc._rotation.numpy())
f64, _ = FR.field(resolution=RES, num_blocks=NB, dtype=np.float64, **ins)
f32, _ = FR.field(resolution=RES, num_blocks=NB, dtype=np.float32, **ins)
rel64, abs64 = FR.distance(occ, f64)
rel32, abs32 = FR.distance(occ, f32)
print("recording vs fp64 restatement: rel %.3e abs %.3e;  vs fp32 restatement: rel %.3e abs %.3e;  max %.4f"
      % (rel64, abs64, rel32, abs32, occ.max()))
path = os.path.join(ROOT, "tests", "golden", "reference_fields.npz")
np.savez_compressed(path, occ=occ, center=pc.center.numpy(), scale=np.float64(pc.scale),
                    meta=np.array([RES, NB, 1.5, rel64, abs64, rel32, abs32], np.float64), **ins)
print("wrote", path, os.path.getsize(path), "bytes")
