"""humangaussian_amd - MI355X-native differentiable 3DGS rasterizer for HumanGaussian.

Only what the rasterize hot path needs:
  csrc/            hand-written HIP kernels (gfx950) + the C ABI of include/hgs_rast.h
  _lib.py          build + ctypes binding of libhgs_rast.so
  rasterizer.py    GaussianRasterizationSettings / GaussianRasterizer (reference API mirror)
  renderer.py      render() / Renderer.render() mirrors (the reference's two call sites)
  view_parallel.py view-parallel multi-GPU rendering (one RCCL all-gather per step)
  step_images.py   guidance_images(): the guidance's two images and the opacity losses of a step
  photometric.py   photometric_loss(): L1 + D-SSIM and PSNR of image fitting; l1_loss / ssim / psnr drop-ins
  surface.py       SurfaceSampler / create_from_pcd: the body surface sampled and the initial Gaussians built on the device
  mesh_view.py     MeshView: the body mesh rasterized forward-only (the animation loop's mesh mode, mesh previews)
  meshclean.py     mesh_components / clean_mesh / decimate_mesh: the extracted mesh without floaters, decimated to a face budget
  synth.py         synthetic SMPL-X-like clouds + threestudio-style cameras (bench/tests)
"""
from .rasterizer import (  # noqa: F401
    GaussianRasterizationSettings,
    GaussianRasterizer,
    rasterize_gaussians,
    rasterize_gaussians_batch,
)

from .meshclean import clean_mesh, decimate_mesh, mesh_components  # noqa: F401
from .photometric import PhotometricLoss, photometric_loss  # noqa: F401
from .step_images import StepImages, guidance_images  # noqa: F401
from .surface import (  # noqa: F401
    SurfaceSampler,
    create_from_pcd,
    create_from_points,
    init_from_body,
    sample_surface,
)

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians",
           "rasterize_gaussians_batch", "StepImages", "guidance_images", "PhotometricLoss", "photometric_loss", "SurfaceSampler", "sample_surface",
           "create_from_points", "create_from_pcd", "init_from_body", "mesh_components", "clean_mesh", "decimate_mesh"]
