"""CPU: the generated marching-cubes case table (tools/gen_mc_table.py ->
csrc/mc_table.h) and the meshes it gives through a pure-numpy walker.

The walker (mesh_helpers.walk) restates the whole extraction of csrc/mesh.hip:
vertices by (lattice point, axis), triangles by (cell, table order)."""
import numpy as np
import pytest

import mesh_helpers as mh
from mesh_helpers import gen


def test_generator_reproduces_the_committed_header():
    assert open(mh.HEADER).read() == gen.render_header()


def _crossed(case):
    return {e for e, (a, b) in enumerate(gen.EDGES) if (case >> a & 1) != (case >> b & 1)}


def _loops_from_face_rule(case):
    """Number of loops, recomputed here from the face rule: per face (corners
    counter-clockwise from outside), one directed segment per run of inside
    corners, from the exit after the run to the entry before it."""
    nxt = {}
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in range(2):
            ring = [(0, 0), (1, 0), (1, 1), (0, 1)]
            ring = ring if side else ring[::-1]
            cs = [side << axis | a << u | b << v for a, b in ring]
            ins = [case >> c & 1 for c in cs]
            for i in range(4):
                if ins[i] and not ins[(i + 1) % 4]:
                    j = i
                    while ins[(j - 1) % 4]:
                        j = (j - 1) % 4
                    key = lambda a, b: gen.EDGE_ID[(min(a, b), max(a, b))]  # noqa: E731
                    nxt[key(cs[i], cs[(i + 1) % 4])] = key(cs[(j - 1) % 4], cs[j])
    seen, loops = set(), 0
    for s in nxt:
        if s not in seen:
            loops += 1
            while s not in seen:
                seen.add(s)
                s = nxt[s]
    return loops, set(nxt)


def test_every_case():
    tab = mh.table()
    assert len(tab) == 256 and not tab[0] and not tab[255]
    assert sum(len(t) for t in tab) == 820
    for case in range(1, 255):
        tris = tab[case]
        assert 1 <= len(tris) <= 5, case
        crossed = _crossed(case)
        loops, chained = _loops_from_face_rule(case)
        assert chained == crossed
        assert len(tris) == len(crossed) - 2 * loops, case
        for t in tris:
            assert set(t) <= crossed and len(set(t)) == 3, (case, t)


def test_edge_numbering_matches_the_header_comment():
    for e, (a, b) in enumerate(gen.EDGES):
        axis = e // 4
        assert b == a | 1 << axis and not a >> axis & 1
        assert gen.EDGE_BASE[e] == a


@pytest.fixture(scope="module")
def noise_meshes():
    return {seed: (mh.noise_volume(seed),) + mh.walk(mh.noise_volume(seed), 0.5) for seed in range(6)}


def test_white_noise_all_cases_occur(noise_meshes):
    seen = set()
    for vol, _, _ in noise_meshes.values():
        seen |= set(np.unique(mh.case_index(vol, 0.5)).tolist())
    assert seen == set(range(256))


@pytest.mark.parametrize("seed", range(6))
def test_white_noise_closed_manifold_outward(noise_meshes, seed):
    vol, verts, faces = noise_meshes[seed]
    if seed < 3:
        assert len(verts) == (4496, 4316, 4380)[seed]
    assert faces.min() >= 0 and faces.max() < len(verts)
    mh.assert_closed_manifold(faces, len(verts))
    assert mh.signed_volume(verts, faces) > 0


@pytest.fixture(scope="module")
def sphere32():
    vol = mh.sphere_volume((32, 32, 32))
    verts, faces = mh.walk(vol, 10.0)
    return vol, mh.lattice_to_world(verts, vol.shape, (-1, -1, -1, 1, 1, 1)).astype(np.float64), faces


def test_sphere(sphere32):
    _, world, faces = sphere32
    r = mh.SPHERE_R
    mh.assert_closed_manifold(faces, len(world))
    assert mh.euler(faces) == 2
    vol, ar = mh.signed_volume(world, faces), mh.area(world, faces)
    print(f"sphere 32^3: volume {vol / (4 / 3 * np.pi * r ** 3) - 1:+.4%} area {ar / (4 * np.pi * r ** 2) - 1:+.4%}")
    assert abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.03
    assert abs(ar / (4 * np.pi * r ** 2) - 1) < 0.03
    h = 2.0 / 31
    off = np.abs(np.linalg.norm(world - mh.SPHERE_C, axis=1) - r).max() / h
    print(f"sphere 32^3: max vertex distance from the sphere {off:.4f} lattice spacings")
    assert off < 0.05


def test_torus_and_two_spheres():
    for vol, chi in ((mh.torus_volume((32, 32, 32)), 0), (mh.two_spheres_volume((32, 32, 32)), 4)):
        verts, faces = mh.walk(vol, 10.0)
        mh.assert_closed_manifold(faces, len(verts))
        assert mh.euler(faces) == chi
        assert mh.signed_volume(verts, faces) > 0
