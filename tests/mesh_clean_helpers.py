"""Shared by the mesh cleaning tests (test_mesh_clean_cpu.py,
test_gpu_mesh_clean.py): numpy restatements of the connected components, the
keep rule with its stable compaction and the colour quantisation, and the
small meshes the kernels are run on. Nothing here needs a GPU."""
import numpy as np


# ---- the yardsticks -----------------------------------------------------------

def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.all((f >= 0) & (f < V), axis=1)


def components_ref(faces, V):
    """-> (labels int32 [V], comp_faces int32 [V]): labels[v] the smallest vertex
    index of v's component, comp_faces[r] the triangles of the component
    labelled r (0 where r is no label). A plain union-find; faces with an index
    outside [0, V) are ignored."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, V)
    parent = list(range(V))

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    for a, b, c in f[ok].tolist():
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)  # the root stays the smallest index of its tree
    labels = np.array([find(v) for v in range(V)], np.int32).reshape(V)
    comp_faces = np.zeros(V, np.int32)
    if ok.any():
        np.add.at(comp_faces, labels[f[ok][:, 0]], 1)
    return labels, comp_faces


def clean_ref(vertices, faces, normals=None, min_faces=0, keep_largest=False):
    """The keep rule and the stable compaction with masks and cumsum ->
    (vertices, faces int32, normals or None, info)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, T = len(v), len(f)
    labels, comp_faces = components_ref(f, V)
    roots = np.nonzero(labels == np.arange(V))[0]
    keep_comp = np.zeros(V, bool)
    keep_comp[roots] = comp_faces[roots] >= min_faces
    if keep_largest and len(roots):
        best = roots[np.argmax(comp_faces[roots])]  # argmax: the first maximum, roots ascend: the smaller label
        only = np.zeros(V, bool)
        only[best] = keep_comp[best]
        keep_comp = only
    ok = valid_faces(f, V)
    keep_f = np.zeros(T, bool)
    keep_f[ok] = keep_comp[labels[f[ok][:, 0]]]
    keep_v = np.zeros(V, bool)
    keep_v[f[keep_f].reshape(-1)] = True
    new_index = np.cumsum(keep_v) - 1  # exclusive position of every kept vertex
    f2 = new_index[f[keep_f]].astype(np.int32).reshape(-1, 3)
    info = dict(components=int(len(roots)), components_kept=int(keep_comp.sum()),
                vertices_dropped=int(V - keep_v.sum()), faces_dropped=int(T - keep_f.sum()))
    n2 = None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3)[keep_v]
    return v[keep_v], f2, n2, info


def colors_ref(logits_f16):
    """255 sigmoid(x) in float64 (not yet truncated), any shape."""
    x = np.asarray(logits_f16, np.float16).astype(np.float64)
    with np.errstate(over="ignore"):
        return 255.0 / (1.0 + np.exp(-x))


# ---- meshes ---------------------------------------------------------------------

def _numbering(V, how, seed):
    if how == "ascending":
        return np.arange(V)
    if how == "descending":
        return np.arange(V)[::-1].copy()
    return np.random.default_rng(seed).permutation(V)


def _finish(faces, V, how, seed, shuffle=True):
    """Renumber the vertices and (seeded) shuffle the face order."""
    f = _numbering(V, how, seed)[np.asarray(faces, np.int64)]
    if shuffle:
        f = f[np.random.default_rng(seed + 1).permutation(len(f))]
    return f.astype(np.int32).reshape(-1, 3), V


def strip(n, how="ascending", seed=0):
    """n triangles (i, i + 1, i + 2): one component of n + 2 vertices."""
    i = np.arange(n)
    return _finish(np.stack([i, i + 1, i + 2], 1), n + 2, how, seed)


def fan(n, hub_last=False):
    """n triangles round one hub, numbered 0 or V - 1; the rim is a closed ring of n vertices."""
    i = np.arange(n)
    V = n + 1
    if hub_last:
        f = np.stack([np.full(n, V - 1), i, (i + 1) % n], 1)
    else:
        f = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1)
    return _finish(f, V, "ascending", 5)


def disjoint_triangles(n, seed=0):
    """n triangles sharing nothing, vertex numbering permuted: n components."""
    return _finish(np.arange(3 * n).reshape(n, 3), 3 * n, "random", seed)


TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])  # closed, outward for a right-handed corner


def two_tetrahedra():
    """V = 8, T = 8: two identical closed components, labels 0 and 4."""
    return np.concatenate([TETRA, TETRA + 4]).astype(np.int32), 8


def with_invalid_faces():
    """A strip of 6 triangles with a face holding index V and one holding -1
    spliced in, and two vertices (8, 9) no triangle uses."""
    f, _ = strip(6, "ascending")
    V = 10
    f = np.concatenate([f[:2], [[0, 3, V]], f[2:4], [[-1, 2, 5]], f[4:]]).astype(np.int32)
    return f, V


def synthetic_meshes():
    """name -> (faces int32 [T, 3], V): every index-only mesh of the GPU tests."""
    out = {
        "empty": (np.zeros((0, 3), np.int32), 0),
        "no_faces": (np.zeros((0, 3), np.int32), 5),
        "one_triangle": (np.array([[0, 1, 2]], np.int32), 3),
        "two_tetrahedra": two_tetrahedra(),
        "fan_hub_first": fan(2000),
        "fan_hub_last": fan(2000, hub_last=True),
        "disjoint_3000": disjoint_triangles(3000),
        "invalid_faces": with_invalid_faces(),
    }
    for n in (63, 64, 65, 4099):
        for how in ("ascending", "descending", "random"):
            out[f"strip_{n}_{how}"] = strip(n, how, seed=n)
    return out


def fake_vertices(V, seed=0):
    """Distinct float32 positions and unit normals for an index-only mesh."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    n = rng.standard_normal((V, 3)).astype(np.float32)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)
    return v, n.astype(np.float32)
