"""Generate morpheus_amd/csrc/mc_table.inc: the marching-cubes triangle table of csrc/mesh.hip and tests/mc_oracle.py.

`python tools/gen_mc_table.py` prints the file; `--write` replaces the committed one (tests/test_mesh_host.py checks that
the two agree).

Numbering is Bourke's ("Polygonising a scalar field"): corner i of the cell at grid point p is
    0 (0,0,0)  1 (1,0,0)  2 (1,1,0)  3 (0,1,0)  4 (0,0,1)  5 (1,0,1)  6 (1,1,1)  7 (0,1,1)      (offsets along x, y, z)
bit i of the case index is set when corner i is inside (f < iso), and edge e joins the corners EDGES[e].

The table is derived from the case geometry rather than typed in, so that one rule settles every ambiguous face:
  * on each face of the cell, the crossed edges are joined in pairs.  A face with 2 crossed edges has one segment; a face
    with 4 (diagonal corners alike) is cut so that each INSIDE corner is separated -- the rule depends on the face's four
    corners alone, so the two cells that share a face draw the same segments there, and closed level sets give closed
    meshes;
  * each segment is directed with the inside corners on its left seen from outside the cell; the directed segments then
    close into loops, and each loop becomes a fan of triangles.  A fan diagonal never joins two vertices of one ambiguous
    face (the neighbour across that face could draw the same pair and the mesh edge would have four triangles).
The winding is Bourke's: (v1 - v0) x (v2 - v0) points toward the inside corners (decreasing f); mesh.hip swaps two indices
when it emits.  Packed form, one 64-bit word per case: the triangles' edge numbers as nibbles from bit 0 up (three per
triangle, at most 15) and the triangle count in bits 60-63.
"""
from __future__ import annotations

import os
import sys

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
# faces: corner cycle and outward normal
FACES = [((0, 1, 2, 3), (0, 0, -1)), ((4, 5, 6, 7), (0, 0, 1)), ((0, 1, 5, 4), (0, -1, 0)),
         ((3, 2, 6, 7), (0, 1, 0)), ((0, 3, 7, 4), (-1, 0, 0)), ((1, 2, 6, 5), (1, 0, 0))]

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "morpheus_amd", "csrc", "mc_table.inc")


def _edge(a, b):
    for e, (u, v) in enumerate(EDGES):
        if {u, v} == {a, b}:
            return e
    raise KeyError((a, b))


def _mid(e):
    u, v = EDGES[e]
    return tuple((CORNERS[u][k] + CORNERS[v][k]) / 2 for k in range(3))


def _sub(a, b):
    return tuple(a[k] - b[k] for k in range(3))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(a[k] * b[k] for k in range(3))


def case_triangles(case: int):
    """-> list of (e0, e1, e2) in Bourke's winding for one case index"""
    inside = [bool(case >> i & 1) for i in range(8)]
    nxt, ambiguous_faces = {}, []
    for cyc, n in FACES:
        fe = [_edge(cyc[i], cyc[(i + 1) % 4]) for i in range(4)]     # face edge i joins cyc[i] and cyc[i+1]
        crossed = [fe[i] for i in range(4) if inside[cyc[i]] != inside[cyc[(i + 1) % 4]]]
        if not crossed:
            continue
        segs = []                                                    # (edge a, edge b, reference corner, its side)
        if len(crossed) == 2:
            ins = [c for c in cyc if inside[c]]
            if len(ins) == 2:
                ref, sign = tuple(sum(CORNERS[c][k] for c in ins) / 2 for k in range(3)), 1
            elif len(ins) == 1:
                ref, sign = CORNERS[ins[0]], 1
            else:
                ref, sign = CORNERS[next(c for c in cyc if not inside[c])], -1
            segs.append((crossed[0], crossed[1], ref, sign))
        else:
            ambiguous_faces.append(set(fe))
            for i in range(4):
                if inside[cyc[i]]:                                   # cut this inside corner off
                    segs.append((fe[(i + 3) % 4], fe[i], CORNERS[cyc[i]], 1))
        for a, b, ref, sign in segs:
            pa = _mid(a)
            side = _dot(_cross(n, _sub(_mid(b), pa)), _sub(ref, pa)) * sign
            assert side != 0
            if side < 0:
                a, b = b, a
            assert a not in nxt, (case, a)
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), case                # every crossed edge: one segment in, one out
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop = [start]
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        n = len(loop)
        for r in range(n):
            v = loop[r:] + loop[:r]
            if not any({v[0], v[i]} <= f for i in range(2, n - 1) for f in ambiguous_faces):
                break
        else:
            raise AssertionError(f"case {case}: no fan start avoids an ambiguous-face diagonal")
        tris += [(v[0], v[i], v[i + 1]) for i in range(1, n - 1)]
    assert len(tris) <= 5, case
    return tris


def packed_table():
    words = []
    for case in range(256):
        tris = case_triangles(case)
        w = len(tris) << 60
        for i, e in enumerate(x for t in tris for x in t):
            w |= e << (4 * i)
        words.append(w)
    return words


def render() -> str:
    words = packed_table()
    lines = ["// Generated by tools/gen_mc_table.py -- do not edit.  Marching-cubes triangle table, one word per case",
             "// (Bourke's corner / edge numbering, bit i = corner i inside): edge nibbles from bit 0, triangle count in bits 60-63."]
    for i in range(0, 256, 4):
        lines.append(" ".join(f"0x{w:016x}ull," for w in words[i:i + 4]))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render()
    if "--write" in sys.argv:
        with open(OUT, "w") as f:
            f.write(text)
        print(OUT)
    else:
        sys.stdout.write(text)
