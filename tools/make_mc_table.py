"""Writes humangaussian_amd/csrc/mc_table.h: the 256-case triangle table of marching cubes, as plain data.

Corner and edge numbering are Lorensen-Cline's as published by Bourke ("Polygonising a scalar field"):
corners 0..7 = (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1); edges 0..11 join the corner pairs of
EDGES below.  Bit i of the case index is set iff corner i is INSIDE (value >= threshold).

The rows are derived, not copied: on each cube face the crossed edges are joined by segments that depend on the four
corner signs of that face alone (two crossed edges: one segment; four: two segments, each cutting off one INSIDE corner),
so two cells that share a face always agree on it and the surface has no holes.  The segments close into loops, a loop of
n edges is cut into n - 2 triangles (no cut lying in a cube face), wound so that the normal points from the inside
corners to the outside ones.
tests/test_fields_cpu.py checks every row of the written header against the cube's geometry."""
import os

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
FACES = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)]   # corners in cyclic order
EDGE_OF = {frozenset(e): i for i, e in enumerate(EDGES)}


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def case_triangles(case):
    inside = [(case >> i) & 1 for i in range(8)]
    links = {}
    for face in FACES:
        fe = [EDGE_OF[frozenset((face[k], face[(k + 1) % 4]))] for k in range(4)]    # edge k joins corners k, k + 1
        crossed = [k for k in range(4) if inside[face[k]] != inside[face[(k + 1) % 4]]]
        if len(crossed) == 2:
            segs = [(fe[crossed[0]], fe[crossed[1]])]
        elif len(crossed) == 4:                                                    # cut off each inside corner
            segs = [(fe[(k - 1) % 4], fe[k]) for k in range(4) if inside[face[k]]]
        else:
            segs = []
        for a, b in segs:
            links.setdefault(a, []).append(b)
            links.setdefault(b, []).append(a)
    assert all(len(v) == 2 for v in links.values())
    mid = [tuple((CORNERS[a][k] + CORNERS[b][k]) / 2 for k in range(3)) for a, b in EDGES]
    tris, todo = [], set(links)
    while todo:
        start = min(todo)
        loop, prev, cur = [start], None, start
        while True:
            todo.discard(cur)
            a, b = links[cur]                       # (two cube edges share at most one face: a != b)
            nxt = b if a == prev else a
            if nxt == start:
                break
            loop.append(nxt)
            prev, cur = cur, nxt
        # Newell normal of the loop against the inside -> outside direction of its edges
        n = (0.0, 0.0, 0.0)
        for k in range(len(loop)):
            n = tuple(x + y for x, y in zip(n, _cross(mid[loop[k]], mid[loop[(k + 1) % len(loop)]])))
        out = 0.0
        for e in loop:
            a, b = EDGES[e]
            d = _sub(CORNERS[b], CORNERS[a]) if inside[a] else _sub(CORNERS[a], CORNERS[b])
            out += _dot(n, d)
        assert out != 0.0
        if out < 0:
            loop = loop[::-1]
        tris += _triangulate(loop)
    return tris


def _coplanar(a, b):
    """Do cube edges a and b lie on one cube face?"""
    return any(set(EDGES[a]) <= set(f) and set(EDGES[b]) <= set(f) for f in FACES)


def _triangulations(poly):
    if len(poly) < 3:
        yield []
        return
    a, b = poly[0], poly[-1]
    for k in range(1, len(poly) - 1):                       # the triangle on the side (last, first)
        for left in _triangulations(poly[:k + 1]):
            for right in _triangulations(poly[k:]):
                yield left + [(a, poly[k], b)] + right


def _triangulate(loop):
    """The first triangulation none of whose interior diagonals lies in a cube face: a diagonal in a face would make a
    triangle flat against the face or meet the neighbouring cell's diagonal there (an edge with four triangles)."""
    sides = {frozenset((loop[k], loop[(k + 1) % len(loop)])) for k in range(len(loop))}
    for tris in _triangulations(loop):
        diag = {frozenset(p) for t in tris for p in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))} - sides
        if not any(_coplanar(*d) for d in diag):
            return [(t[2], t[0], t[1]) for t in tris]      # (a, p, b) keeps the loop's direction: b -> a is its closing side
    raise AssertionError(loop)


def main():
    rows = [case_triangles(c) for c in range(256)]
    width = 3 * max(len(r) for r in rows) + 1
    assert width <= 16, width
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(here, "..", "humangaussian_amd", "csrc", "mc_table.h")
    with open(path, "w") as f:
        f.write("// mc_table.h - the 256 cases of marching cubes (written by tools/make_mc_table.py; data only).\n"
                "// Bit i of the case: corner i is inside (value >= threshold).  Corners 0..7 = (0,0,0) (1,0,0) (1,1,0) (0,1,0)\n"
                "// (0,0,1) (1,0,1) (1,1,1) (0,1,1) as (x,y,z) offsets; edge e joins the corners HGS_MC_EDGE_CORNERS[e].\n"
                "// A row lists the cube edges of its triangles, three per triangle, -1 ends it; normals point inside -> outside.\n"
                "#pragma once\n"
                "#define HGS_MC_ROW 16\n"
                "#ifndef HGS_MC_TABLE_QUAL   /* device code: __constant__ static const */\n"
                "#define HGS_MC_TABLE_QUAL static const\n"
                "#endif\n"
                "HGS_MC_TABLE_QUAL signed char HGS_MC_EDGE_CORNERS[12][2] = {\n  "
                + ", ".join("{%d, %d}" % e for e in EDGES) + "};\n"
                "HGS_MC_TABLE_QUAL signed char HGS_MC_TRI_TABLE[256][HGS_MC_ROW] = {\n")
        for c, r in enumerate(rows):
            flat = [e for t in r for e in t]
            flat += [-1] * (16 - len(flat))
            f.write("  {" + ", ".join("%2d" % v for v in flat) + "},\n")
        f.write("};\n")
    print("wrote", os.path.normpath(path), "max triangles per case:", (width - 1) // 3)


if __name__ == "__main__":
    main()
