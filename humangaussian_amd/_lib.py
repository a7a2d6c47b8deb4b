"""Build + load the two in-tree shared objects:

  libhgs_rast.so   the C-ABI HIP library (include/hgs_rast.h), hipcc for gfx950; bound here
                   through ctypes (`load()`: sizing functions, raw-ABI tests)
  _hgs_torch.so    the torch binding above it (csrc/torch_binding.cpp, g++, no device code):
                   the C++ autograd node the Python API calls (`load_binding()`)

There is no JIT cache and no fallback: if a shared object is missing or does not export the
ABI, importing the rasterizer fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, Structure, c_float, c_int32, c_int64, c_size_t, c_uint8, c_uint32, c_void_p

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG_DIR, "csrc")
LIB_PATH = os.environ.get("HGS_LIB") or os.path.join(_PKG_DIR, "libhgs_rast.so")   # HGS_LIB: A/B experiments only
ABI_VERSION = 17

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
               "-shared"]


class HgsSettings(Structure):
    """ctypes mirror of `hgs_settings` (field order = GaussianRasterizationSettings)."""
    _fields_ = [
        ("image_height", c_int32), ("image_width", c_int32),
        ("tanfovx", c_float), ("tanfovy", c_float),
        ("bg", c_void_p), ("scale_modifier", c_float),
        ("viewmatrix", c_void_p), ("projmatrix", c_void_p),
        ("sh_degree", c_int32), ("campos", c_void_p),
        ("prefiltered", c_int32), ("debug", c_int32),
    ]


class HgsAdamTensor(Structure):
    """ctypes mirror of `hgs_adam_tensor`."""
    _fields_ = [
        ("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
        ("rows", c_int64), ("row_floats", c_int32),
        ("step_size", c_float), ("bc2_sqrt", c_float), ("w1", c_float), ("beta2", c_float), ("w2", c_float),
        ("eps", c_float),
    ]


ADAM_MAX_TENSORS = 16


class HgsAdamArgs(Structure):
    """ctypes mirror of `hgs_adam_args` (the kernel argument of hgs_adam_step)."""
    _fields_ = [
        ("num_tensors", c_int32), ("visible_rows", c_int64), ("visible", c_void_p),
        ("t", HgsAdamTensor * ADAM_MAX_TENSORS), ("block_start", c_uint32 * (ADAM_MAX_TENSORS + 1)),
    ]


class HgsLbsArgs(Structure):
    """ctypes mirror of `hgs_lbs_args` (hgs_lbs_pose)."""
    _fields_ = [
        ("V", c_int32), ("J", c_int32), ("F", c_int32), ("K", c_int32),
        ("weight_width", c_int32), ("posedirs_stride", c_int32),
        ("v_shaped", c_void_p), ("J_rest", c_void_p), ("parents", c_void_p), ("posedirs", c_void_p),
        ("weight_joint", c_void_p), ("weight_value", c_void_p), ("poses", c_void_p), ("transl", c_void_p),
        ("centre", c_float * 3), ("scale", c_float),
        ("workspace", c_void_p), ("vertices", c_void_p), ("joints", c_void_p),
    ]


LBS_MAX_JOINTS = 64
LBS_FRAME_TILE = 8


POSE_OPENPOSE, POSE_HUMANSD = 0, 1
POSE_MAX_LIMBS, POSE_MAX_COLOURS, POSE_RECORD_INTS, POSE_MAX_DIM = 17, 18, 8, 4096


class HgsPoseArgs(Structure):
    """ctypes mirror of `hgs_pose_args` (hgs_pose_draw)."""
    _fields_ = [
        ("style", c_int32), ("B", c_int32), ("K", c_int32), ("H", c_int32), ("W", c_int32),
        ("limb_width", c_int32), ("uint8_out", c_int32), ("num_limbs", c_int32),
        ("points", c_void_p), ("mvp", c_void_p), ("occlusion", c_void_p), ("image", c_void_p), ("kp", c_void_p),
        ("records", c_void_p),
        ("limb", (c_int32 * 3) * POSE_MAX_LIMBS), ("colour", (c_uint8 * 3) * POSE_MAX_COLOURS),
    ]


SI_PIXELS_PER_THREAD, SI_PIXELS_PER_WORKGROUP, SI_PARTIALS_PER_VIEW, SI_MAX_DIM = 4, 1024, 256, 32768


class HgsStepImagesArgs(Structure):
    """ctypes mirror of `hgs_step_images_args` (hgs_step_images_forward / _backward)."""
    _fields_ = [
        ("B", c_int32), ("H", c_int32), ("W", c_int32), ("h", c_int32), ("w", c_int32), ("half_images", c_int32),
        ("render", c_void_p), ("depth", c_void_p), ("workspace", c_void_p), ("rgb_out", c_void_p), ("depth_out", c_void_p),
        ("loss_sparsity", c_void_p), ("loss_opaque", c_void_p), ("depth_min", c_void_p), ("depth_max", c_void_p),
        ("depth_global_max", c_void_p), ("tie_counts", c_void_p),
        ("grad_rgb", c_void_p), ("grad_depth", c_void_p), ("grad_loss_sparsity", c_void_p), ("grad_loss_opaque", c_void_p),
        ("grad_render", c_void_p), ("grad_depth_in", c_void_p),
    ]


PM_TILE_H, PM_TILE_W, PM_FINISH_CHUNK = 32, 32, 64
PM_WINDOW = (0.00102838012, 0.00759875821, 0.0360007733, 0.109360687, 0.213005528, 0.266011715,
             0.213005528, 0.109360687, 0.0360007733, 0.00759875821, 0.00102838012)     # HGS_PM_WINDOW, to be read as fp32


class HgsPhotometricArgs(Structure):
    """ctypes mirror of `hgs_photometric_args` (hgs_photometric_forward / _backward)."""
    _fields_ = [
        ("B", c_int32), ("C", c_int32), ("H", c_int32), ("W", c_int32), ("with_grad", c_int32), ("psnr_per_plane", c_int32),
        ("weight_l1", c_float), ("weight_dssim", c_float),
        ("image", c_void_p), ("gt", c_void_p), ("workspace", c_void_p),
        ("loss", c_void_p), ("l1", c_void_p), ("ssim", c_void_p), ("ssim_image", c_void_p), ("sqerr", c_void_p), ("psnr", c_void_p),
        ("grad_loss", c_void_p), ("grad_l1", c_void_p), ("grad_ssim", c_void_p), ("grad_ssim_image", c_void_p),
        ("grad_image", c_void_p),
    ]


class HgsFsampleArgs(Structure):
    """ctypes mirror of `hgs_fsample_args` (hgs_fsample)."""
    _fields_ = [
        ("info_host", c_void_p), ("axis", c_void_p), ("plan", c_void_p), ("lists", c_void_p),
        ("M", c_int32), ("normalized", c_int32), ("points", c_void_p), ("colors", c_void_p), ("scratch", c_void_p),
        ("density", c_void_p), ("normal", c_void_p), ("color", c_void_p),
    ]


SURFACE_MAX_FACES = (1 << 20) - 1


class HgsSurfaceInfo(Structure):
    """ctypes mirror of `hgs_surface_info` (the 16 bytes hgs_surface_cdf leaves on the device)."""
    _fields_ = [("area", ctypes.c_double), ("num_positive", c_uint32), ("reserved", c_uint32)]


class HgsSurfaceSampleArgs(Structure):
    """ctypes mirror of `hgs_surface_sample_args` (hgs_surface_sample)."""
    _fields_ = [
        ("V", c_int32), ("F", c_int32), ("vertices", c_void_p), ("faces", c_void_p), ("cdf", c_void_p),
        ("N", c_int64), ("offset", ctypes.c_uint64), ("seed", ctypes.c_uint64),
        ("points", c_void_p), ("face", c_void_p), ("uvw", c_void_p),
    ]


MESHVIEW_MAX_DIM, MESHVIEW_TILE, MESHVIEW_LIST_BATCH, MESHVIEW_MAX_ATTR = 4096, 16, 256, 8


class HgsMeshviewInfo(Structure):
    """ctypes mirror of `hgs_meshview_info` (the 32 bytes hgs_meshview_plan leaves on the device)."""
    _fields_ = [("num_refs", ctypes.c_uint64), ("B", c_int32), ("V", c_int32), ("F", c_int32), ("H", c_int32), ("W", c_int32),
                ("reserved", c_uint32)]


class HgsMeshviewArgs(Structure):
    """ctypes mirror of `hgs_meshview_args` (hgs_meshview_normals / _plan / _draw / _interpolate)."""
    _fields_ = [
        ("B", c_int32), ("V", c_int32), ("F", c_int32), ("H", c_int32), ("W", c_int32),
        ("C", c_int32), ("shade_normals", c_int32), ("background", c_float),
        ("vertex_stride", c_int64), ("attr_stride", c_int64),
        ("vertices", c_void_p), ("mvp", c_void_p), ("faces", c_void_p), ("adj_start", c_void_p), ("adj", c_void_p),
        ("attr", c_void_p), ("rast_in", c_void_p), ("records", c_void_p), ("plan", c_void_p), ("lists", c_void_p),
        ("info", c_void_p), ("rast", c_void_p), ("image", c_void_p), ("normals", c_void_p),
    ]


MESHCLEAN_G_MAX, MESHCLEAN_MAX_ITEMS = 1024, 1 << 29


class HgsMeshcleanInfo(Structure):
    """ctypes mirror of `hgs_meshclean_info` (the 64 bytes the hgs_meshclean_* calls keep on the device)."""
    _fields_ = [("bmin", c_uint32 * 3), ("bmax", c_uint32 * 3), ("bad_faces", c_uint32), ("error", c_uint32),
                ("num_vertices", c_uint32), ("num_faces", c_uint32), ("reserved", c_uint32 * 6)]


class HgsMeshcleanArgs(Structure):
    """ctypes mirror of `hgs_meshclean_args` (every hgs_meshclean_* call)."""
    _fields_ = [
        ("V", c_int32), ("F", c_int32), ("vertices", c_void_p), ("faces", c_void_p), ("scratch", c_void_p),
        ("info", c_void_p), ("labels", c_void_p), ("comp_faces", c_void_p), ("comp_diag2", c_void_p),
        ("min_f", c_int32), ("min_d", c_float), ("vertices_out", c_void_p), ("faces_out", c_void_p),
        ("vertex_src", c_void_p),
    ]


class HgsStatus(Structure):
    _fields_ = [
        ("num_rendered", c_uint32), ("active_tiles", c_uint32), ("num_pairs", c_uint32),
        ("bwd_groups", c_uint32), ("overflow", c_uint32), ("reserved", c_uint32 * 3),
    ]


EXPORTS = {
    "hgs_abi_version": (ctypes.c_int, []),
    "hgs_geom_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "hgs_bin_bytes": (c_size_t, [c_int64]),
    "hgs_img_bytes": (c_size_t, [c_int32, c_int32]),
    "hgs_bwd_scratch_bytes": (c_size_t, [c_int64]),
    "hgs_bwd_scratch_bytes_pairs": (c_size_t, [c_int64, c_int64]),
    "hgs_geom_bytes_batch": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "hgs_img_bytes_batch": (c_size_t, [c_int32, c_int32, c_int32]),
    "hgs_forward_batch": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_int32, c_int32] + [c_void_p] * 7
                          + [c_void_p] * 4 + [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32,
                                              c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "hgs_backward_batch": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_int32, c_int32] + [c_void_p] * 8
                           + [c_void_p] * 6 + [c_void_p] * 3 + [POINTER(HgsStatus), c_int64, c_void_p]
                           + [c_void_p] * 8 + [c_void_p, c_void_p]),
    "hgs_forward_batch_act": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_int32, c_int32] + [c_void_p] * 7
                              + [c_void_p] * 4 + [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32,
                                                  c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "hgs_forward_batch_act_leaf": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_int32, c_int32] + [c_void_p] * 7
                                   + [c_void_p] * 4 + [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32,
                                                       c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "hgs_backward_batch_act": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_int32, c_int32] + [c_void_p] * 8
                               + [c_void_p] * 6 + [c_void_p] * 3 + [POINTER(HgsStatus), c_int64, c_void_p]
                               + [c_void_p] * 8 + [c_void_p, c_int32, c_void_p]),
    "hgs_forward": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_int32] + [c_void_p] * 7
                    + [c_void_p] * 4 + [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32,
                                        c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "hgs_backward": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_int32] + [c_void_p] * 8
                     + [c_void_p] * 6 + [c_void_p] * 3 + [POINTER(HgsStatus), c_int64, c_void_p]
                     + [c_void_p] * 8 + [c_void_p, c_void_p]),
    "hgs_mark_visible": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_void_p, c_void_p,
                                        c_void_p]),
    "hgs_knn_mean_dist2": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p]),
    "hgs_knn_scratch_bytes": (c_size_t, [c_int32]),
    "hgs_knn_mean_dist2_grid": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hgs_reduce_view_packs": (ctypes.c_int, [c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "hgs_reduce_view_packs_acc": (ctypes.c_int, [c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hgs_pack_view_contribution": (ctypes.c_int, [c_int32, c_int32] + [c_void_p] * 9),
    "hgs_backward_batch_packed": (ctypes.c_int, [POINTER(HgsSettings), c_int32, c_int32, c_int32] + [c_void_p] * 5
                                  + [c_void_p] * 7 + [c_void_p] * 3 + [POINTER(HgsStatus), c_int64, c_void_p]
                                  + [c_void_p] * 2 + [c_void_p, c_int32, c_void_p]),
    "hgs_reduce_view_packs_unpack": (ctypes.c_int, [c_int32, c_int64, c_int32] + [c_void_p] * 9 + [c_void_p]),
    "hgs_densify_stats": (ctypes.c_int, [c_int32, c_int32] + [c_void_p] * 9),
    "hgs_densify_masks": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p]
                          + [c_float] * 6 + [c_void_p] * 5),
    "hgs_compact_scratch_bytes": (c_size_t, [c_int32]),
    "hgs_compact_index": (ctypes.c_int, [c_int32] + [c_void_p] * 5),
    "hgs_gather_rows": (ctypes.c_int, [c_int64, c_int32] + [c_void_p] * 4),
    "hgs_reanchor": (ctypes.c_int, [c_int32] + [c_void_p] * 7),
    "hgs_reanchor_rot": (ctypes.c_int, [c_int32] + [c_void_p] * 6 + [c_int32] + [c_void_p] * 3),
    "hgs_adam_step": (ctypes.c_int, [POINTER(HgsAdamArgs), c_void_p]),
    "hgs_lbs_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "hgs_lbs_pose": (ctypes.c_int, [POINTER(HgsLbsArgs), c_void_p]),
    "hgs_pose_records_bytes": (c_size_t, [c_int32, c_int32]),
    "hgs_pose_draw": (ctypes.c_int, [POINTER(HgsPoseArgs), c_void_p]),
    "hgs_step_images_workspace_bytes": (c_size_t, [c_int32] * 5),
    "hgs_step_images_forward": (ctypes.c_int, [POINTER(HgsStepImagesArgs), c_void_p]),
    "hgs_step_images_backward": (ctypes.c_int, [POINTER(HgsStepImagesArgs), c_void_p]),
    "hgs_photometric_workspace_bytes": (c_size_t, [c_int32] * 5),
    "hgs_photometric_forward": (ctypes.c_int, [POINTER(HgsPhotometricArgs), c_void_p]),
    "hgs_photometric_backward": (ctypes.c_int, [POINTER(HgsPhotometricArgs), c_void_p]),
    "hgs_mesh_grid_plan": (ctypes.c_int, [c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "hgs_mesh_grid_bytes": (c_size_t, [c_void_p]),
    "hgs_mesh_grid_build": (ctypes.c_int, [c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hgs_mesh_query": (ctypes.c_int, [c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "hgs_field_plan_bytes": (c_size_t, [c_int32, c_int32]),
    "hgs_field_plan": (ctypes.c_int, [c_int32] + [c_void_p] * 4 + [c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p,
                                                               c_void_p]),
    "hgs_field_list_bytes": (c_size_t, [c_void_p]),
    "hgs_field_eval": (ctypes.c_int, [c_void_p] * 7),
    "hgs_mc_scratch_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "hgs_mc_count": (ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p]),
    "hgs_mc_emit": (ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_float] + [c_void_p] * 5),
    "hgs_fsample_scratch_bytes": (c_size_t, [c_int32, c_int32]),
    "hgs_fsample": (ctypes.c_int, [POINTER(HgsFsampleArgs), c_void_p]),
    "hgs_surface_cdf_scratch_bytes": (c_size_t, [c_int32]),
    "hgs_surface_cdf": (ctypes.c_int, [c_int32, c_void_p, c_int32] + [c_void_p] * 5),
    "hgs_surface_sample": (ctypes.c_int, [POINTER(HgsSurfaceSampleArgs), c_void_p]),
    "hgs_init_gaussians": (ctypes.c_int, [c_int64, c_int32] + [c_void_p] * 9),
    "hgs_meshview_plan_bytes": (c_size_t, [c_int32] * 4),
    "hgs_meshview_normals": (ctypes.c_int, [POINTER(HgsMeshviewArgs), c_void_p]),
    "hgs_meshview_plan": (ctypes.c_int, [POINTER(HgsMeshviewArgs), c_void_p]),
    "hgs_meshview_list_bytes": (c_size_t, [POINTER(HgsMeshviewInfo)]),
    "hgs_meshview_draw": (ctypes.c_int, [POINTER(HgsMeshviewArgs), POINTER(HgsMeshviewInfo), c_void_p]),
    "hgs_meshview_interpolate": (ctypes.c_int, [POINTER(HgsMeshviewArgs), c_void_p]),
    "hgs_meshclean_scratch_bytes": (c_size_t, [c_int32, c_int32]),
    "hgs_meshclean_begin": (ctypes.c_int, [POINTER(HgsMeshcleanArgs), c_void_p]),
    "hgs_meshclean_rounds": (ctypes.c_int, [POINTER(HgsMeshcleanArgs), c_int32, c_void_p, c_void_p]),
    "hgs_meshclean_components": (ctypes.c_int, [POINTER(HgsMeshcleanArgs), c_void_p]),
    "hgs_meshclean_clean_mark": (ctypes.c_int, [POINTER(HgsMeshcleanArgs), c_void_p]),
    "hgs_meshclean_clean_emit": (ctypes.c_int, [POINTER(HgsMeshcleanArgs), POINTER(HgsMeshcleanInfo), c_void_p]),
    "hgs_meshclean_count": (ctypes.c_int, [POINTER(HgsMeshcleanArgs), POINTER(c_int32), c_void_p, c_void_p]),
    "hgs_meshclean_decimate_mark": (ctypes.c_int, [POINTER(HgsMeshcleanArgs), c_int32, c_void_p]),
    "hgs_meshclean_decimate_emit": (ctypes.c_int, [POINTER(HgsMeshcleanArgs), POINTER(HgsMeshcleanInfo), c_void_p]),
}


BINDING_SRC = "torch_binding.cpp"
BINDING_PATH = os.path.join(_PKG_DIR, "_hgs_torch.so")


def sources():
    return [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f != BINDING_SRC]


def needs_build() -> bool:
    target = os.path.join(_PKG_DIR, "libhgs_rast.so")
    if not os.path.exists(target):
        return True
    mt = os.path.getmtime(target)
    deps = sources() + [os.path.join(_PKG_DIR, "..", "include", "hgs_rast.h")]
    return any(os.path.getmtime(s) > mt for s in deps)


# translation units: (source, extra flags)
UNITS = [("api.hip", []),
         ("render_bwd.hip", [])]


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the translation units for gfx950 with hipcc and link libhgs_rast.so."""
    target = os.path.join(_PKG_DIR, "libhgs_rast.so")
    if not force and not needs_build():
        return target
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libhgs_rast.so")
    common = [f for f in HIPCC_FLAGS if f != "-shared"]
    objs = []
    for src, extra in UNITS:
        obj = os.path.join(_PKG_DIR, "_build_" + src.replace(".hip", ".o"))
        cmd = [hipcc] + common + extra + ["-c", os.path.join(_CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + res.stdout + res.stderr)
        objs.append(obj)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", target + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + res.stdout + res.stderr)
    os.replace(target + ".tmp", target)
    for o in objs:
        os.remove(o)
    return target


def binding_needs_build() -> bool:
    if not os.path.exists(BINDING_PATH):
        return True
    mt = os.path.getmtime(BINDING_PATH)
    deps = [os.path.join(_CSRC, BINDING_SRC), os.path.join(_PKG_DIR, "..", "include", "hgs_rast.h")]
    return any(os.path.getmtime(s) > mt for s in deps)


def build_binding(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/torch_binding.cpp with g++ against this interpreter's torch and link it to
    libhgs_rast.so (rpath $ORIGIN).  Host code only: hipcc is not involved."""
    if not force and not binding_needs_build():
        return BINDING_PATH
    import sysconfig
    import torch
    from torch.utils import cpp_extension as ce
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("g++ not found: cannot build _hgs_torch.so")
    tlib = ce.library_paths()[0]
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-DTORCH_EXTENSION_NAME=_hgs_torch",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}"]
    cmd += [f"-I{p}" for p in ce.include_paths()] + [f"-I{rocm_inc}", f"-I{sysconfig.get_paths()['include']}"]
    cmd += [os.path.join(_CSRC, BINDING_SRC), "-o", BINDING_PATH + ".tmp", f"-L{tlib}", "-lc10", "-lc10_hip",
            "-ltorch_cpu", "-ltorch_hip", "-ltorch", "-ltorch_python", f"-L{_PKG_DIR}", "-lhgs_rast",
            f"-Wl,-rpath,{tlib}", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("g++ failed for torch_binding.cpp:\n" + res.stdout + res.stderr)
    os.replace(BINDING_PATH + ".tmp", BINDING_PATH)
    return BINDING_PATH


_binding = None


def load_binding():
    """Import humangaussian_amd/_hgs_torch.so (the C++ autograd node).  Fails loudly."""
    global _binding
    if _binding is not None:
        return _binding
    load()                                   # ABI check of libhgs_rast.so first
    if not os.path.exists(BINDING_PATH):
        raise ImportError(
            f"{BINDING_PATH} is missing: the torch binding has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback for the product path.")
    import importlib.util
    import torch  # noqa: F401  (libtorch must be loaded before the extension)
    spec = importlib.util.spec_from_file_location("humangaussian_amd._hgs_torch", BINDING_PATH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.abi_version() != ABI_VERSION:
        raise ImportError(f"{BINDING_PATH}: linked against ABI {mod.abi_version()} != {ABI_VERSION}")
    _binding = mod
    return mod


_lib = None


def load() -> ctypes.CDLL:
    """dlopen the library and bind every symbol include/hgs_rast.h declares."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP rasterizer extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise ImportError(f"{LIB_PATH} does not export {name}")
        fn.restype = res
        fn.argtypes = args
    if lib.hgs_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.hgs_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib
