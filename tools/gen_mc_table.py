#!/usr/bin/env python3
"""Derive the marching-cubes case table and write torch-ngp_amd/csrc/mc_table.h.

Pure Python, no dependencies. The table is constructed, not copied (DESIGN
§11):

  corner  c = x + 2y + 4z; a corner is inside when value >= threshold.
  edge    e = 4 * axis + r: the corner pair (base, base | 1 << axis), where
          base is the r-th corner (ascending) whose `axis` bit is clear. The
          edge belongs to the lattice point at the cell's minimum corner plus
          base's offsets, along `axis`.
  face    its 4 corners counter-clockwise seen from outside the cell. Walking
          that boundary, a crossed edge is an exit (inside -> outside) or an
          entry (outside -> inside). Every inside corner that is followed by
          an outside one is cut off by one directed segment, from the exit
          after its run of inside corners to the entry before it: one segment
          for 2 crossings, two for the ambiguous face (inside corners on a
          diagonal, each cut off on its own). The rule reads the face's four
          flags only, so both cells sharing a face draw the same segments.
  loops   every crossed edge is the exit of one of its two faces and the entry
          of the other; following exit -> entry closes the segments into loops.
  fill    a loop of n vertices takes n - 2 triangles: the first triangulation
          (in a fixed enumeration) none of whose diagonals joins two cell
          edges of a common face. Such a diagonal lies in the face plane and
          the neighbouring cell could draw it too (a mesh edge used 4 times).
  orient  each triangle is reversed, so normals point from inside to outside.

Usage: python tools/gen_mc_table.py [--check] [output]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(ROOT, "torch-ngp_amd", "csrc", "mc_table.h")
MAX_TRIS = 5

# edge id -> (corner a, corner b), a < b, differing in bit `axis`
EDGES = []
for _axis in range(3):
    for _base in range(8):
        if not _base >> _axis & 1:
            EDGES.append((_base, _base | 1 << _axis))
EDGE_ID = {pair: e for e, pair in enumerate(EDGES)}
EDGE_AXIS = [e // 4 for e in range(12)]
EDGE_BASE = [a for a, _ in EDGES]


def _faces():
    """The 6 faces as 4 corners, counter-clockwise seen from outside."""
    faces = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3  # e_u x e_v = e_axis
        for side in range(2):
            ring = [(0, 0), (1, 0), (1, 1), (0, 1)]  # counter-clockwise about +axis
            if side == 0:
                ring = ring[::-1]
            faces.append([side << axis | a << u | b << v for a, b in ring])
    return faces


FACES = _faces()
FACE_SETS = [frozenset(f) for f in FACES]


def edge_of(a, b):
    return EDGE_ID[(min(a, b), max(a, b))]


def share_face(e0, e1):
    """Do two cell edges lie on a common face?"""
    need = set(EDGES[e0]) | set(EDGES[e1])
    return any(need <= f for f in FACE_SETS)


def face_segments(flags):
    """flags: inside flag of a face's 4 corners in ring order -> directed
    segments as (exit ring-edge, entry ring-edge); ring-edge i joins corner i
    and corner i + 1."""
    segs = []
    for i in range(4):
        if flags[i] and not flags[(i + 1) % 4]:  # ring-edge i is an exit
            j = i
            while flags[(j - 1) % 4]:  # back over this run of inside corners
                j = (j - 1) % 4
                if j == i:
                    break
            segs.append((i, (j - 1) % 4))
    return segs


def case_segments(case):
    """Directed segments (exit cell-edge -> entry cell-edge) of a case."""
    out = {}
    for ring in FACES:
        flags = [case >> c & 1 for c in ring]
        for ex, en in face_segments(flags):
            e_exit = edge_of(ring[ex], ring[(ex + 1) % 4])
            e_entry = edge_of(ring[en], ring[(en + 1) % 4])
            assert e_exit not in out, "an edge is the exit of one face only"
            out[e_exit] = e_entry
    return out


def case_loops(case):
    nxt = case_segments(case)
    crossed = {e for e, (a, b) in enumerate(EDGES) if (case >> a & 1) != (case >> b & 1)}
    assert set(nxt) == crossed and set(nxt.values()) == crossed
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def _triangulations(idx):
    """Every triangulation of the polygon idx (a list of positions), as lists
    of position triples, in a fixed order."""
    if len(idx) < 3:
        yield []
        return
    a, b = idx[0], idx[-1]
    for m in range(1, len(idx) - 1):
        for left in _triangulations(idx[:m + 1]):
            for right in _triangulations(idx[m:]):
                yield left + [(a, idx[m], b)] + right


def fill_loop(loop):
    n = len(loop)
    for tris in _triangulations(list(range(n))):
        ok = True
        for t in tris:
            for p, q in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                if (q - p) % n in (1, n - 1):
                    continue  # a polygon side
                if share_face(loop[p], loop[q]):
                    ok = False
        if ok:
            return [(loop[t[0]], loop[t[1]], loop[t[2]]) for t in tris]
    raise AssertionError(f"no admissible triangulation of loop {loop}")


def build_table():
    """-> list of 256 lists of triangles (edge-id triples), oriented with the
    normal from inside to outside."""
    table = []
    for case in range(256):
        tris = []
        for loop in case_loops(case):
            tris += [(a, c, b) for a, b, c in fill_loop(loop)]  # reversed
        assert len(tris) <= MAX_TRIS
        table.append(tris)
    assert not table[0] and not table[255]
    assert sum(len(t) for t in table) == 820
    return table


def render_header(table=None):
    table = build_table() if table is None else table
    lines = [
        "// Marching-cubes case table. GENERATED by tools/gen_mc_table.py: do not edit,",
        "// rerun the generator (tests/test_mesh_table.py compares byte for byte).",
        "//   corner c = x + 2y + 4z, inside when value >= threshold (bit c of the case);",
        "//   edge e = 4 * axis + r: from the r-th corner whose `axis` bit is clear, along axis;",
        "//   kMcTris[case]: up to 5 triangles as edge ids, -1 padded, normals inside -> outside.",
        "//   NGP_MC_TABLE_ATTR: the including file's storage attribute (__device__ in csrc/mesh.hip).",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#ifndef NGP_MC_TABLE_ATTR",
        "#define NGP_MC_TABLE_ATTR",
        "#endif",
        "",
        "#define NGP_MC_MAX_TRIS 5",
        "#define NGP_MC_TOTAL_TRIS 820",
        "",
        "NGP_MC_TABLE_ATTR static const uint8_t kMcTriCount[256] __attribute__((aligned(16))) = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(table[c])) for c in range(r, r + 32)) + ",")
    lines += ["};", "", "NGP_MC_TABLE_ATTR static const int8_t kMcTris[256][16] __attribute__((aligned(16))) = {"]
    for c in range(256):
        flat = [e for t in table[c] for e in t]
        flat += [-1] * (16 - len(flat))
        lines.append("    {" + ", ".join(f"{e:2d}" for e in flat) + "},  // " + f"{c:3d}")
    lines += ["};", ""]
    return "\n".join(lines)


def main(argv):
    args = [a for a in argv if a != "--check"]
    out = args[0] if args else DEFAULT_OUT
    text = render_header()
    if "--check" in argv:
        same = os.path.exists(out) and open(out).read() == text
        print("up to date" if same else "STALE", out)
        return 0 if same else 1
    with open(out, "w") as f:
        f.write(text)
    print(f"wrote {out}: 256 cases, 820 triangles")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
