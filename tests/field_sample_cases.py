"""The cases of the point-sampling tests (tests/test_field_sample_cpu.py, tests/test_gpu_field_sample.py): three of the
clouds of tests/test_gpu_fields.py, and per cloud the points the field is sampled at - the vertices of its own mesh and
2 000 uniform points of the grid's box grown by 10 %, in normalised coordinates and in world coordinates.  Pure numpy."""
import functools

import numpy as np

import field_sample_reference as SR
import fields_reference as FR

CASES = ("fixture", "dense", "sparse")
UNIFORM = 2000
NEAR_CAP = 1e-3


def cloud_of(case):
    import test_gpu_fields as G
    make, res, nb = G.CASES[case]
    return make(), res, nb


def threshold(field_max):
    """The iso-value of a case's mesh: the reference's 1 where the field reaches it, else 0.3 of the maximum."""
    return float(min(1.0, 0.3 * field_max))


def colors_of(n, seed=77):
    return np.random.default_rng(seed).uniform(0, 1, size=(n, 3)).astype(np.float32)


def uniform_points(case):
    """UNIFORM points of [-1.1, 1.1]^3 (normalised): inside the grid, and beyond every face of it (edge blocks)."""
    return np.random.default_rng(1000 + CASES.index(case)).uniform(-1.1, 1.1, size=(UNIFORM, 3)).astype(np.float32)


def vertices_normalised(vertices_index, resolution):
    """Index coordinates -> normalised ones, in fp32 as fields.extract_mesh does it."""
    return (np.asarray(vertices_index, np.float32) / np.float32(resolution - 1.0) * np.float32(2) - np.float32(1)).astype(np.float32)


def to_world(n, center, scale):
    """fp32, as fields.extract_mesh: n / scale + center."""
    return (np.asarray(n, np.float32) / np.float32(scale) + np.asarray(center, np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def restated_mesh(case):
    """(vertices in index coordinates, faces, fp64 Prepared) of the case's mesh from the restatement alone."""
    cloud, res, nb = cloud_of(case)
    occ, P = FR.field(*cloud, resolution=res, num_blocks=nb, dtype=np.float64)
    v, f = FR.weld(FR.marching_cubes(occ, threshold(occ.max())))
    return v, f, P


def on_plane(n, P):
    """Points with a coordinate within SR.NEAR of a plane between two blocks (what SR.sample flags as `near`)."""
    planes = P.axis[np.arange(1, P.num_blocks) * P.split].astype(np.float64)
    return (np.abs(np.asarray(n, np.float64)[:, :, None] - planes[None, None, :]) < SR.NEAR).any((1, 2))


# ------------------------------------------------------------------------------------------------ the mesh test's cloud

ELLIPSOID = dict(n=4000, seed=7, scale0=0.04, spread=0.3, resolution=32, num_blocks=16)    # extract_mesh's num_blocks
RED, BLUE = np.array([1.0, 0.0, 0.0], np.float32), np.array([0.0, 0.0, 1.0], np.float32)


def ellipsoid_cloud():
    """FR.cloud's ellipsoid (long axis z) with scales wide enough for a smooth surface at resolution 32."""
    return FR.cloud(ELLIPSOID["n"], ELLIPSOID["seed"], scale0=ELLIPSOID["scale0"], spread=ELLIPSOID["spread"])


def two_colours(cloud):
    """(P,3): red for the Gaussians of the upper half (z > 0), blue for the lower."""
    return np.where((cloud[0][:, 2] > 0)[:, None], RED, BLUE).astype(np.float32)


def far_from_seam(world, cloud):
    """+1 / -1 for points more than three times the cloud's largest standard deviation above / below z = 0, else 0."""
    reach = 3.0 * float(cloud[2].max())
    z = np.asarray(world, np.float64)[:, 2]
    return np.where(z > reach, 1, np.where(z < -reach, -1, 0))


# ------------------------------------------------------------------------------------------------ reading a mesh PLY back

def read_mesh_ply(path):
    """(vertex rows as a structured array, faces (T,3), vertex property names) of ply_io.save_mesh_ply's file."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    nv = nf = None
    props, target = [], None
    for ln in lines[2:-1]:
        tok = ln.split()
        if tok[0] == "element":
            target = tok[1]
            if target == "vertex":
                nv = int(tok[2])
            else:
                assert target == "face"
                nf = int(tok[2])
        elif tok[0] == "property" and target == "vertex":
            props.append((tok[2], {"float": "<f4", "uchar": "u1"}[tok[1]]))
        elif tok[0] == "property":
            assert tok[1:] == ["list", "uchar", "int", "vertex_indices"]
    v = np.frombuffer(data, dtype=props, count=nv, offset=end)
    f = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + v.nbytes)
    assert end + v.nbytes + f.nbytes == len(data)
    assert (f["n"] == 3).all()
    return v, f["i"], [p[0] for p in props]
