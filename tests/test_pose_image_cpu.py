"""CPU tests of the pose-control images' host side (no GPU): the integer rasteriser of tests/pose_reference.py against
float64 evaluations of the same shapes, the palette, the trig table and the blend rule against their definitions, the
tables of humangaussian_amd/pose_image.py against the reference's literals (when its tree is there), the sampler of the
GPU records test, the two new exports of the C ABI and their argument validation, which launches nothing."""
import ast
import colorsys
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pose_reference as pr
from humangaussian_amd import _lib
from humangaussian_amd import pose_image as pi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_POSER = os.path.join(os.environ.get("HGS_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference"),
                               "threestudio", "utils", "poser.py")
MARGIN = 1e-9
# the views the GPU records test draws (tests/test_gpu_pose_image.py uses the same table)
RECORD_CASES = [("openpose", 64, 64, 3, 11), ("openpose", 97, 130, 8, 12), ("openpose", 512, 512, 8, 13),
                ("humansd", 64, 64, 3, 21), ("humansd", 97, 130, 8, 22), ("humansd", 512, 512, 8, 23)]


# ------------------------------------------------------------------------------------ the rasteriser's integer tests

CAPSULES = [(5, 7, 40, 30, 1), (5, 7, 40, 30, 2), (5, 7, 40, 30, 7), (30, 20, 30, 20, 7), (30, 20, 30, 20, 1), (10, 40, 50, 40, 10),
            (20, 5, 20, 45, 9), (-12, -9, 70, 60, 6), (60, 3, 2, 44, 3), (25, 25, 26, 25, 8), (100, 100, 200, 90, 5)]


@pytest.mark.parametrize("cap", CAPSULES)
def test_integer_capsule_agrees_with_float64_geometry(cap):
    H, W = 52, 75
    rec = np.array([pr.CAPSULE, *cap, 0, 0], np.int64)
    got = pr.covered(rec, H, W, crop=False)
    assert np.array_equal(got, pr.covered(rec, H, W))                      # the rasteriser's window loses nothing
    m = pr.capsule_margin(rec, H, W)
    clear = np.abs(m) > MARGIN
    assert np.array_equal(got[clear], (m <= 0)[clear])
    # what lies on the boundary in float64 is decided by the integers: 4 d^2 = w^2 is covered
    assert clear.sum() > 0.9 * H * W
    if cap[:2] == cap[2:4]:            # length 0: the disc of diameter w
        py, px = np.mgrid[0:H, 0:W]
        assert np.array_equal(got, 4 * ((px - cap[0]) ** 2 + (py - cap[1]) ** 2) <= cap[4] ** 2)
    if max(cap[0], cap[2]) < W and max(cap[1], cap[3]) < H and min(cap[:4]) >= 0:
        assert got[cap[1], cap[0]] and got[cap[3], cap[2]]                 # the end points themselves (x = column, y = row)


ELLIPSES = [(30, 25, a, th) for a in (0, 1, 3, 4, 5, 17) for th in (0, 1, 37, 45, 89, 90, 91, 135, 180, -1, -45, -90, -135, -179, -180)] \
    + [(3, 2, 30, 20), (70, 50, 12, -60), (37, 26, 40, 33)]


@pytest.mark.parametrize("ell", ELLIPSES, ids=[f"c{e[0]}_{e[1]}_a{e[2]}_t{e[3]}" for e in ELLIPSES])
def test_integer_ellipse_agrees_with_float64_geometry(ell):
    H, W = 52, 75
    cx, cy, a, theta = ell
    rec = np.array([pr.ELLIPSE, cx, cy, a, theta, 4, 0, 0], np.int64)
    got = pr.covered(rec, H, W, crop=False)
    assert np.array_equal(got, pr.covered(rec, H, W))                      # the rasteriser's window loses nothing
    m, degenerate = pr.ellipse_margin(rec, H, W)
    clear = np.abs(m) > MARGIN
    assert np.array_equal(got[clear], (m <= 0)[clear])
    assert clear.sum() > 0.9 * H * W
    if 0 <= cx < W and 0 <= cy < H:
        assert got[cy, cx]                                                 # the centre is always inside
    if degenerate:
        # a = 0 keeps the pixels with u = 0 exactly: a line of at most 2 b + 1 pixels on the axes and diagonals, the
        # centre alone at other angles whose fixed-point (C, S) has no small integer null vector
        assert 1 <= got.sum() <= 9
        if theta % 90 == 0:
            assert got.sum() == 9
    else:
        # the half axes: a along (cos, sin) theta, 4 across - the extreme pixels on the axes are inside for axis angles
        if theta % 180 == 0 and cx - a >= 0 and cx + a < W:
            assert got[cy, cx - a] and got[cy, cx + a] and (cx + a + 1 >= W or not got[cy, cx + a + 1])
            assert got[cy - 4, cx] and got[cy + 4, cx] and not got[cy + 5, cx]


def test_third_ellipse_test_stays_below_2_to_58_and_capsule_below_2_to_63():
    """the bounds of the header: coordinates <= 8191, pixels < 4096, width <= 32767, a < 2^12, b = 4"""
    d = 8191 + 4095
    assert 4 * (2 * d * d) ** 2 < 2 ** 63 and 32767 ** 2 * (2 * (2 * 8191) ** 2) < 2 ** 63
    a = int(np.sqrt(2) * 4096 / 2) + 1
    assert a < 2 ** 12 and (a * pr.ONE) ** 2 * 16 + (4 * pr.ONE) ** 2 * a * a < 2 ** 58
    assert 2 * d * pr.ONE < 2 ** 31                  # u and v fit int32 for any pixel and a centre inside the image


def test_disc_is_dx2_plus_dy2_le_16():
    rec = np.array([pr.DISC, 10, 12, 16, 0, 0, 0, 0], np.int64)
    got = pr.covered(rec, 30, 30)
    assert got.sum() == 49 and got[12, 14] and got[16, 10] and not got[16, 11] and got[15, 12] and not got[15, 13]


# ------------------------------------------------------------------------------------------------------- the tables

def test_palette_matches_colorsys():
    hues = np.linspace(0, 1, 17)[:-1] + 0.01
    want = tuple(tuple(int(255 * c) for c in colorsys.hls_to_rgb(h, 0.6, 0.65)) for h in hues)
    assert pi.HUMANSD_COLOURS == want == pi.hls_palette(16)
    assert want[:3] == ((219, 94, 86), (219, 144, 86), (219, 194, 86))
    # no channel is close enough to an integer for the last bits of colorsys to matter
    assert min(abs(255 * c - round(255 * c)) for h in hues for c in colorsys.hls_to_rgb(h, 0.6, 0.65)) > 1e-3
    # and the library's own copy (csrc/api.hip)
    src = open(os.path.join(ROOT, "humangaussian_amd", "csrc", "api.hip")).read()
    body = re.search(r"POSE_COLOURS_HUMANSD\[16\]\[3\] = \{(.*?)\};", src, flags=re.S).group(1)
    assert tuple(tuple(int(v) for v in t.split(",")) for t in re.findall(r"\{([^{}]*)\}", body)) == want


def _c_table(name, src):
    body = re.search(name + r"\[\d+\]\[3\] = \{(.*?)\};", src, flags=re.S).group(1)
    return tuple(tuple(int(v) for v in t.split(",")) for t in re.findall(r"\{([^{}]*)\}", body))


def test_library_tables_equal_the_module_tables():
    src = open(os.path.join(ROOT, "humangaussian_amd", "csrc", "api.hip")).read()
    assert _c_table("POSE_LIMBS_HUMANSD", src) == pi.HUMANSD_LIMBS and _c_table("POSE_LIMBS_OPENPOSE", src) == pi.OPENPOSE_LIMBS
    assert _c_table("POSE_COLOURS_OPENPOSE", src) == pi.OPENPOSE_COLOURS
    assert len(pi.HUMANSD_LIMBS) == 16 and len(pi.OPENPOSE_LIMBS) == 17 and len(pi.OPENPOSE_COLOURS) == 18


def test_trig_table_matches_rint():
    hdr = open(os.path.join(ROOT, "humangaussian_amd", "csrc", "pose_trig.h")).read()
    vals = [int(v) for v in re.findall(r"-?\d+", hdr.split("HGS_POSE_COS[360] = {")[1].split("}")[0])]
    want = np.rint(16384 * np.cos(np.radians(np.arange(360)))).astype(int).tolist()
    assert vals == want == pr.TRIG and len(vals) == 360
    assert "#define HGS_POSE_TRIG_ONE 16384" in hdr
    # the sine is the cosine a quarter turn back; C^2 + S^2 stays within the bound the kernel's culling box relies on
    for k in range(360):
        assert pr.TRIG[(k - 90) % 360] == int(np.rint(16384 * np.sin(np.radians(k)))) or k % 90 == 0
        assert abs(pr.TRIG[k] ** 2 + pr.TRIG[(k - 90) % 360] ** 2 - 2 ** 28) <= 23171


def test_blend_rule_is_round_of_addweighted_for_all_pairs():
    c, k = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = (4 * c + 6 * k + 5) // 10
    assert np.array_equal(got, np.rint(0.4 * c + 0.6 * k).astype(int))
    assert ((2 * (2 * c + 3 * k)) % 10 != 5).all()     # (2 c + 3 k) / 5 has no fractional part of one half: never on a tie
    assert got.min() == 0 and got.max() == 255


@pytest.mark.skipif(not os.path.exists(REFERENCE_POSER), reason="the reference tree is not present")
def test_tables_equal_the_reference_literals():
    tree = ast.parse(open(REFERENCE_POSER).read())
    found = {}

    class V(ast.NodeVisitor):
        def visit_Assign(self, node):
            t = node.targets[0]
            name = t.id if isinstance(t, ast.Name) else (t.attr if isinstance(t, ast.Attribute) else None)
            if name in ("humansd_skeleton", "indices", "colors", "lines", "name"):
                try:
                    val = node.value
                    if isinstance(val, ast.BinOp):                              # np.array([...]) - 1
                        val = val.left
                    if isinstance(val, ast.Call):
                        val = val.args[0]
                    found.setdefault(name, []).append(ast.literal_eval(val))
                except (ValueError, IndexError):
                    pass
            self.generic_visit(node)

    V().visit(tree)
    assert tuple(tuple(r) for r in found["humansd_skeleton"][0]) == pi.HUMANSD_LIMBS
    assert tuple(tuple(r) for r in found["colors"][0]) == pi.OPENPOSE_COLOURS
    openpose_map, humansd_map = found["indices"]
    assert tuple(i - 1 for i in openpose_map) == pi.SMPLX_TO_OPENPOSE18 and tuple(i - 1 for i in humansd_map) == pi.SMPLX_TO_HUMANSD17
    names = [tuple(n) for n in found["name"]]
    assert pi.HUMANSD_NAMES in names and pi.OPENPOSE_NAMES in names
    lines = [tuple(tuple(r) for r in ln) for ln in found["lines"]]
    assert pi.HUMANSD_LINES in lines and pi.OPENPOSE_LINES in lines


def test_keypoints_from_joints_selects_by_name():
    j = np.arange(60 * 3, dtype=np.float32).reshape(60, 3)
    kp = pi.keypoints_from_joints(j, "openpose")
    assert kp.shape == (18, 3) and kp[0, 0] == 55 * 3 and kp[1, 0] == 12 * 3 and kp[4, 0] == 21 * 3 and kp[17, 0] == 59 * 3
    kh = pi.keypoints_from_joints(torch.from_numpy(j)[None], "humansd")
    assert kh.shape == (1, 17, 3) and kh[0, 1, 0] == 57 * 3 and kh[0, 2, 0] == 56 * 3 and kh[0, 16, 0] == 8 * 3
    assert np.array_equal(pi.keypoints_from_joints(j, True), kh[0].numpy())
    with pytest.raises(ValueError):
        pi.keypoints_from_joints(j[:59], "openpose")
    with pytest.raises(ValueError):
        pi.keypoints_from_joints(j, "coco")


# ------------------------------------------------------------------------------------- the reference's two halves

def test_fp32_restatement_stays_close_to_fp64():
    for style, H, W, B, seed in RECORD_CASES:
        points, mvp, _ = pr.sample_views(style, H, W, B, seed)
        for b in range(B):
            r64, k64, _ = pr.records_of(style, points, mvp[b], H, W, occlusion=True)
            r32, k32, _ = pr.records_of(style, points, mvp[b], H, W, occlusion=True, dtype=np.float32)
            assert np.abs(k32.astype(np.float64) - k64)[:, :2].max() <= 16 * pr.EPS32 * max(H, W)
            assert np.array_equal(r32, r64)           # the sampler's margin: fp32 truncates as float64 does


@pytest.mark.parametrize("case", RECORD_CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}_B{c[3]}" for c in RECORD_CASES])
def test_sampler_fills_its_quota_with_the_committed_seed(case):
    style, H, W, B, seed = case
    points, mvp, tries = pr.sample_views(style, H, W, B, seed)
    print(case, "draws:", tries)
    assert mvp.shape == (B, 4, 4) and mvp.dtype == np.float32 and tries <= pr.SAMPLER_TRIES
    drawn = 0
    for b in range(B):
        vals = pr.fragile_values(style, points, mvp[b], H, W)
        assert np.abs(vals - np.rint(vals)).min() >= pr.SAMPLER_MARGIN
        rec, kp, _ = pr.records_of(style, points, mvp[b], H, W)
        drawn += int((rec[:, 0] != 0).sum())
        assert np.isfinite(kp).all()
    assert drawn >= B * pr.NUM_RECORDS[style] * 0.8           # the skeletons are in view: the comparison is not vacuous


def test_hand_built_view_rasterises_to_what_the_rules_say():
    """two crossing HumanSD limbs: the later one wins where they overlap; an OpenPose limb blends 0.6 of its colour"""
    recs = np.zeros((16, 8), np.int64)
    recs[2] = [pr.CAPSULE, 5, 20, 45, 20, 5, 0, pr.rgb((10, 20, 30))]
    recs[9] = [pr.CAPSULE, 25, 2, 25, 40, 5, 0, pr.rgb((200, 100, 50))]
    img = pr.rasterise(recs, 48, 52)
    assert tuple(img[20, 25]) == (200, 100, 50) and tuple(img[20, 10]) == (10, 20, 30) and tuple(img[5, 25]) == (200, 100, 50)
    assert tuple(img[0, 0]) == (0, 0, 0)
    swapped = recs.copy()
    swapped[[2, 9]] = recs[[9, 2]]
    assert tuple(pr.rasterise(swapped, 48, 52)[20, 25]) == (10, 20, 30)
    e = np.zeros((35, 8), np.int64)
    e[0] = [pr.DISC, 20, 20, 16, 0, 0, 0, pr.rgb((255, 0, 0))]
    e[18] = [pr.ELLIPSE, 20, 20, 10, 0, 4, 0, pr.rgb((255, 0, 0))]
    e[19] = [pr.ELLIPSE, 20, 20, 10, 90, 4, 0, pr.rgb((255, 85, 0))]
    img = pr.rasterise(e, 48, 52)
    assert tuple(img[20, 20]) == (255, round(0.6 * 85), 0)                  # disc, then two blends
    assert tuple(img[20, 29]) == (round(0.6 * 255), 0, 0)                   # the first limb alone over black
    assert np.array_equal(pr.to_float(img), img.astype(np.float32) / np.float32(255))
    assert pr.to_float(np.array([255, 0, 51], np.uint8)).tolist() == [1.0, 0.0, float(np.float32(0.2))]


# ------------------------------------------------------------------------------------------------------------ the ABI

def test_abi_exports_and_argument_validation_without_a_gpu():
    hdr = open(os.path.join(ROOT, "include", "hgs_rast.h")).read()
    assert re.search(r"^int hgs_pose_draw\(const hgs_pose_args\* args, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^size_t hgs_pose_records_bytes\(int32_t style, int32_t B\);", hdr, flags=re.M)
    for name, val in (("OPENPOSE", _lib.POSE_OPENPOSE), ("HUMANSD", _lib.POSE_HUMANSD), ("MAX_LIMBS", _lib.POSE_MAX_LIMBS),
                      ("MAX_COLOURS", _lib.POSE_MAX_COLOURS), ("RECORD_INTS", _lib.POSE_RECORD_INTS), ("MAX_DIM", _lib.POSE_MAX_DIM)):
        assert int(re.search(r"#define HGS_POSE_%s (\d+)" % name, hdr).group(1)) == val
    assert "hgs_pose_draw" in _lib.EXPORTS and "hgs_pose_records_bytes" in _lib.EXPORTS
    _lib.build()
    lib = _lib.load()
    assert lib.hgs_abi_version() == 17 == _lib.ABI_VERSION
    fields = re.search(r"typedef struct hgs_pose_args \{(.*?)\} hgs_pose_args;", hdr, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\w+\])*\s*[,;]", fields)
    assert names == [f[0] for f in _lib.HgsPoseArgs._fields_]
    assert _lib.HgsPoseArgs.points.offset == 32 and _lib.HgsPoseArgs.limb.offset == 80
    assert _lib.HgsPoseArgs.colour.offset == 284 and ctypes.sizeof(_lib.HgsPoseArgs) == 344

    assert lib.hgs_pose_records_bytes(_lib.POSE_HUMANSD, 3) == 3 * 16 * 32 and lib.hgs_pose_records_bytes(_lib.POSE_OPENPOSE, 1) == 35 * 32
    assert lib.hgs_pose_records_bytes(2, 1) == 0 and lib.hgs_pose_records_bytes(0, -1) == 0 and lib.hgs_pose_records_bytes(0, 0) == 0

    def call(**kw):
        """a call whose every pointer is non-NULL (never dereferenced: each variant below is refused, or has B = 0)"""
        a = _lib.HgsPoseArgs()
        a.style, a.B, a.K, a.H, a.W, a.limb_width = _lib.POSE_OPENPOSE, 0, 18, 64, 64, 1
        for name in ("points", "mvp", "occlusion", "image", "kp", "records"):
            setattr(a, name, 4096)
        limbs = kw.pop("limbs", None)
        for k, v in kw.items():
            setattr(a, k, v)
        if limbs is not None:
            a.num_limbs = len(limbs)
            for i, row in enumerate(limbs):
                for c in range(3):
                    a.limb[i][c] = row[c]
        return lib.hgs_pose_draw(ctypes.byref(a), None)

    OK, EINVAL = 0, -1
    assert lib.hgs_pose_draw(None, None) == EINVAL
    assert call() == OK                                                                     # B = 0
    assert call(style=_lib.POSE_HUMANSD, K=17) == OK
    assert call(K=17) == EINVAL and call(style=_lib.POSE_HUMANSD, K=18) == EINVAL and call(K=0) == EINVAL
    assert call(style=2) == EINVAL and call(style=-1) == EINVAL
    assert call(B=-1) == EINVAL and call(B=65536) == EINVAL
    assert call(H=0) == EINVAL and call(W=0) == EINVAL and call(H=4097) == EINVAL and call(W=4097) == EINVAL and call(H=-5) == EINVAL
    assert call(H=4096, W=4096) == OK and call(H=1, W=1) == OK
    assert call(limb_width=0) == EINVAL and call(limb_width=-3) == EINVAL and call(limb_width=32768) == EINVAL
    assert call(limb_width=32767) == OK
    assert call(limbs=[(0, 0, 1)]) == OK and call(limbs=[(0, 0, 18)]) == EINVAL and call(limbs=[(18, 0, 1)]) == EINVAL
    assert call(limbs=[(0, -1, 1)]) == EINVAL and call(num_limbs=18) == EINVAL and call(num_limbs=-1) == EINVAL
    assert call(style=_lib.POSE_HUMANSD, K=17, num_limbs=17) == EINVAL
    for name in ("points", "mvp", "image", "kp", "records"):                                # refused before any launch
        assert call(B=2, **{name: None}) == EINVAL, name
    _lib.build_binding()
    doc = _lib.load_binding().pose_draw.__doc__
    for arg in ("points", "mvp", "occlusion", "style", "H", "W", "limb_width", "uint8_out"):
        assert arg in doc
    with pytest.raises(RuntimeError, match="HIP device"):
        _lib.load_binding().pose_draw(torch.zeros(18, 4), torch.zeros(1, 4, 4), None, 0, 64, 64, 1, False)


def test_pose_skeleton_refuses_cpu_tensors_and_a_cpu_device():
    with pytest.raises(RuntimeError, match="HIP device"):
        pi.PoseSkeleton(np.zeros((18, 3), np.float32), device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        pi.PoseSkeleton(torch.zeros(18, 3))
    assert {"draw_views", "draw", "humansd_draw", "hand_centers", "from_joints", "from_body"} <= set(dir(pi.PoseSkeleton))
    assert pi.default_limb_width(512) == 10 and pi.default_limb_width(52) == 1 and pi.default_limb_width(51) == 0
