"""CPU: the yardsticks of the mesh cleaning tests (mesh_clean_helpers.py) held
to scipy and to mesh properties, and the PLY writer / reader with colours."""
import numpy as np
import pytest

import mesh_clean_helpers as mc
import mesh_helpers as mh
from nerf.mesh import read_ply, write_ply


def _walked(name):
    if name == "noise":
        return mh.walk(mh.noise_volume(0, 16), 0.5)
    return mh.walk(mh.two_spheres_volume((24, 24, 24)), 10.0)


@pytest.fixture(scope="module", params=["noise", "two_spheres"])
def walked(request):
    v, f = _walked(request.param)
    return request.param, v, f


def test_components_ref_matches_scipy(walked):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    name, v, f = walked
    V = len(v)
    labels, comp_faces = mc.components_ref(f, V)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]]])
    g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
    n, want = connected_components(g, directed=False)
    assert len(np.unique(labels)) == n
    if name == "noise":
        assert n >= 24  # dozens of components
    else:
        assert n == 2
    # the same partition: each of our classes is one of scipy's, and the counts agree
    pairs = np.unique(np.stack([labels.astype(np.int64), want.astype(np.int64)], 1), axis=0)
    assert len(pairs) == n
    # every label is the minimum of its class
    for r in np.unique(labels):
        assert r == np.nonzero(labels == r)[0].min()
    # the triangle counts: every face once, on its component's label
    assert comp_faces.sum() == len(f)
    assert np.array_equal(np.nonzero(comp_faces)[0], np.unique(labels[f[:, 0]]))
    assert np.array_equal(comp_faces[np.unique(labels)], np.bincount(labels[f[:, 0]], minlength=V)[np.unique(labels)])


def test_components_ref_ignores_invalid_faces_and_isolated_vertices():
    f, V = mc.with_invalid_faces()
    labels, comp_faces = mc.components_ref(f, V)
    assert labels.tolist() == [0] * 8 + [8, 9]
    assert comp_faces.tolist() == [6] + [0] * 9


@pytest.mark.parametrize("min_faces", [1, 2, 50])
def test_clean_ref_keeps_a_closed_manifold(walked, min_faces):
    _, v, f = walked
    mh.assert_closed_manifold(f, len(v))
    v2, f2, _, info = mc.clean_ref(v, f, min_faces=min_faces)
    labels, comp_faces = mc.components_ref(f, len(v))
    assert info["components"] == len(np.unique(labels))
    assert info["components_kept"] == int((comp_faces[np.unique(labels)] >= min_faces).sum())
    assert info["vertices_dropped"] == len(v) - len(v2) and info["faces_dropped"] == len(f) - len(f2)
    if len(f2):
        assert f2.min() == 0 and f2.max() == len(v2) - 1  # every kept vertex is used
        mh.assert_closed_manifold(f2, len(v2))
    # stable: the kept vertices are a subsequence of the input
    kept = np.zeros(len(v), bool)
    kept[np.unique(f[comp_faces[labels[f[:, 0]]] >= min_faces])] = True
    assert np.array_equal(v2.view(np.uint32), v[kept].view(np.uint32))


def test_clean_ref_keep_largest_of_two_spheres():
    """Radii 0.3 and 0.2: the larger one alone is left, a sphere (Euler characteristic 2)."""
    x = mh.lattice((24, 24, 24))
    vol = np.maximum(mh.blob(np.linalg.norm(x - np.array([-0.45, 0.0, 0.0]), axis=-1), 0.3),
                     mh.blob(np.linalg.norm(x - np.array([0.45, 0.1, 0.0]), axis=-1), 0.2))
    v, f = mh.walk(vol, 10.0)
    labels, comp_faces = mc.components_ref(f, len(v))
    assert len(np.unique(labels)) == 2
    v2, f2, _, info = mc.clean_ref(v, f, keep_largest=True)
    assert info["components"] == 2 and info["components_kept"] == 1
    assert len(f2) == comp_faces.max() and 0 < len(v2) < len(v)
    mh.assert_closed_manifold(f2, len(v2))
    assert mh.euler(f2) == 2
    assert np.all(v2[:, 0] < 11.5)  # lattice units: the sphere at x = -0.45 is in the lower half of 0..23


def test_clean_ref_tie_goes_to_the_smaller_label():
    f, V = mc.two_tetrahedra()
    v, _ = mc.fake_vertices(V)
    v2, f2, _, info = mc.clean_ref(v, f, keep_largest=True)
    assert np.array_equal(f2, mc.TETRA) and np.array_equal(v2, v[:4]) and info["components_kept"] == 1


def test_colors_ref_values():
    x = np.array([0.0, np.inf, -np.inf, 11.0], np.float16)
    s = mc.colors_ref(x)
    assert s[0] == 127.5 and s[1] == 255.0 and s[2] == 0.0 and 254.99 < s[3] < 255.0


# ---- PLY with colours -----------------------------------------------------------

def _mesh(seed, V, T):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    n = rng.standard_normal((V, 3)).astype(np.float32)
    f = rng.integers(0, max(V, 1), (T, 3)).astype(np.int32)
    c = rng.integers(0, 256, (V, 3)).astype(np.uint8)
    return v, f, n, c


# V = 37: 37 * 27 = 999 and 37 * 15 = 555 bytes of vertices, so the face records start unaligned
@pytest.mark.parametrize("V,T", [(37, 55), (0, 0), (4, 2)])
@pytest.mark.parametrize("with_normals", [False, True])
def test_coloured_round_trip_is_exact(tmp_path, V, T, with_normals):
    v, f, n, c = _mesh(3, V, T)
    path, again = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    write_ply(path, v, f, n if with_normals else None, colors=c)
    rv, rf, rn, rc = read_ply(path, with_colors=True)
    assert rv.dtype == np.float32 and rf.dtype == np.int32 and rc.dtype == np.uint8
    assert rv.shape == (V, 3) and rf.shape == (T, 3) and rc.shape == (V, 3)
    assert np.array_equal(rv.view(np.uint32), v.view(np.uint32)) and np.array_equal(rf, f) and np.array_equal(rc, c)
    if with_normals:
        assert np.array_equal(rn.view(np.uint32), n.view(np.uint32))
    else:
        assert rn is None
    write_ply(again, rv, rf, rn, colors=rc)
    data = open(path, "rb").read()
    assert data == open(again, "rb").read()
    header, payload = data.split(b"end_header\n")
    lines = header.decode("ascii").split("\n")
    assert lines[-4:-1] == ["property uchar blue", f"element face {T}", "property list uchar int vertex_indices"]
    assert "property uchar red" in lines and lines.index("property uchar red") > lines.index("property float z")
    assert len(payload) == V * (12 * (2 if with_normals else 1) + 3) + T * 13
    # read the old way: the same three, the colours ignored
    three = read_ply(path)
    assert len(three) == 3 and np.array_equal(three[0], rv) and np.array_equal(three[1], rf)


def test_colourless_file_reads_with_colours_as_none(tmp_path):
    v, f, n, _ = _mesh(4, 9, 5)
    path = str(tmp_path / "m.ply")
    write_ply(path, v, f, n)
    out = read_ply(path, with_colors=True)
    assert len(out) == 4 and out[3] is None and np.array_equal(out[0], v)


def test_bad_colours_are_refused(tmp_path):
    v, f, n, c = _mesh(5, 6, 2)
    with pytest.raises(ValueError, match="colors"):
        write_ply(str(tmp_path / "m.ply"), v, f, n, colors=c[:5])
    with pytest.raises(ValueError, match="colors"):
        write_ply(str(tmp_path / "m.ply"), v, f, n, colors=c.astype(np.float32))


def _parent_write_ply(path, vertices, faces, normals=None):
    """write_ply as it stood before colours existed, restated."""
    v = np.ascontiguousarray(np.asarray(vertices, "<f4").reshape(-1, 3))
    f = np.asarray(faces, "<i4").reshape(-1, 3)
    props = ["x", "y", "z"]
    if normals is not None:
        n = np.asarray(normals, "<f4").reshape(-1, 3)
        v = np.ascontiguousarray(np.concatenate([v, n], 1))
        props += ["nx", "ny", "nz"]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property float {p}" for p in props]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    rec["n"] = 3
    rec["v"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("V,T", [(37, 55), (0, 0)])
def test_colourless_file_is_the_parents_bytes(tmp_path, V, T, with_normals):
    v, f, n, _ = _mesh(6, V, T)
    a, b = str(tmp_path / "new.ply"), str(tmp_path / "old.ply")
    write_ply(a, v, f, n if with_normals else None)
    _parent_write_ply(b, v, f, n if with_normals else None)
    assert open(a, "rb").read() == open(b, "rb").read()
