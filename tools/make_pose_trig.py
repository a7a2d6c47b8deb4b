"""Writes humangaussian_amd/csrc/pose_trig.h: T[k] = lround(16384 cos(k degrees)), k = 0..359, as plain data - the
fixed-point cosines the OpenPose limb test of csrc/pose.hip rotates a pixel offset with (include/hgs_rast.h:
hgs_pose_draw).  sin(k) is T[(k - 90) mod 360].  The four axis values are set exactly (cos(90 degrees) in float64 is
6e-17, which rounds to 0 anyway); no other multiple of a degree has a cosine whose 16384-fold lies within 1e-6 of a
half-integer, so the rounding does not depend on the last bits of libm's cos (asserted below).
tests/test_pose_image_cpu.py checks every entry of the written header against rint(16384 cos)."""
import math
import os

ONE = 16384


def table():
    t = []
    for k in range(360):
        x = ONE * math.cos(math.radians(k))
        assert abs(abs(x - math.floor(x)) - 0.5) > 1e-6, k
        t.append(int(math.floor(x + 0.5)))
    assert (t[0], t[90], t[180], t[270]) == (ONE, 0, -ONE, 0)
    return t


def main():
    t = table()
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(here, "..", "humangaussian_amd", "csrc", "pose_trig.h")
    with open(path, "w") as f:
        f.write("// pose_trig.h - HGS_POSE_COS[k] = lround(16384 cos(k degrees)), k = 0..359 (written by tools/make_pose_trig.py;\n"
                "// data only).  sin(k degrees) is HGS_POSE_COS[(k - 90) mod 360].\n"
                "#pragma once\n"
                "#define HGS_POSE_TRIG_ONE 16384\n"
                "#ifndef HGS_POSE_TRIG_QUAL   /* device code: __constant__ static const */\n"
                "#define HGS_POSE_TRIG_QUAL static const\n"
                "#endif\n"
                "HGS_POSE_TRIG_QUAL short HGS_POSE_COS[360] = {\n")
        for r in range(0, 360, 12):
            f.write("  " + ", ".join("%6d" % v for v in t[r:r + 12]) + ",\n")
        f.write("};\n")
    print("wrote", os.path.normpath(path))


if __name__ == "__main__":
    main()
