"""Shared by the mesh tests (test_mesh_table.py, test_gpu_mesh.py): the table
generator as a module, the test volumes, and mesh property checks in numpy."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, "tools", "gen_mc_table.py")
HEADER = os.path.join(ROOT, "torch-ngp_amd", "csrc", "mc_table.h")


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", GENERATOR)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = load_generator()
_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = gen.build_table()
    return _TABLE


def tri_counts():
    return np.array([len(t) for t in table()], np.int64)


# ---- volumes ---------------------------------------------------------------

def noise_volume(seed, n=16):
    """n^3, the inner (n-2)^3 uniform [0, 1) float32, a zero border."""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, n, n), np.float32)
    v[1:-1, 1:-1, 1:-1] = rng.random((n - 2, n - 2, n - 2), dtype=np.float32)
    return v


def lattice(shape, lo=-1.0, hi=1.0):
    axes = [np.linspace(lo, hi, n) for n in shape]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1)


def blob(d, r):
    """20 exp(-ln2 (d/r)^2): crosses 10 at d = r."""
    return (20.0 * np.exp(-np.log(2.0) * (d / r) ** 2)).astype(np.float32)


SPHERE_C, SPHERE_R = np.array([0.013, -0.021, 0.007]), 0.6


def sphere_volume(shape):
    return blob(np.linalg.norm(lattice(shape) - SPHERE_C, axis=-1), SPHERE_R)


def torus_volume(shape, R=0.55, r=0.25):
    x = lattice(shape)
    d = np.sqrt((np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) - R) ** 2 + x[..., 2] ** 2)
    return blob(d, r)


def two_spheres_volume(shape, r=0.3):
    x = lattice(shape)
    d = np.minimum(np.linalg.norm(x - np.array([-0.45, 0.0, 0.0]), axis=-1),
                   np.linalg.norm(x - np.array([0.45, 0.1, 0.0]), axis=-1))
    return blob(d, r)


# ---- the vertex rule (no table) ---------------------------------------------

def inside_mask(vol, thr):
    with np.errstate(invalid="ignore"):
        return vol >= np.float32(thr)


def crossed_edges(vol, thr):
    """-> (p, axis) of every crossed lattice edge in (p, axis) order, and the
    per-point 3-bit flags [nx, ny, nz]."""
    ins = inside_mask(vol, thr)
    flags = np.zeros(vol.shape, np.uint8)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        flags[tuple(lo)] |= (ins[tuple(lo)] != ins[tuple(hi)]).astype(np.uint8) << a
    f = flags.reshape(-1)
    bits = (f[:, None] >> np.arange(3)[None]) & 1
    p, axis = np.nonzero(bits)  # row-major: p ascending, then axis
    return p.astype(np.int64), axis.astype(np.int64), flags


def vertex_rule(vol, thr, p, axis):
    """The fp32 vertex formula: t = (thr - a) / (b - a), pos = p0 + t (p1 - p0)
    in lattice units, a at p and b at its +axis neighbour (NaN read as 0)."""
    nx, ny, nz = vol.shape
    f32 = np.float32
    v = np.where(np.isnan(vol), f32(0), vol).reshape(-1)
    stride = np.array([ny * nz, nz, 1], np.int64)
    a, b = v[p], v[p + stride[axis]]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((f32(thr) - a) / (b - a)).astype(f32)
    ijk = np.stack([p // (ny * nz), p // nz % ny, p % nz], -1)
    p0 = ijk.astype(f32)
    p1 = (ijk + np.eye(3, dtype=np.int64)[axis]).astype(f32)
    return (p0 + t[:, None] * (p1 - p0)).astype(f32)


def lattice_to_world(pos, shape, aabb):
    """min + (max - min) * (pos / (n - 1)) per axis, in fp32."""
    f32 = np.float32
    mn, mx = np.asarray(aabb[:3], f32), np.asarray(aabb[3:], f32)
    den = (np.asarray(shape, np.int64) - 1).astype(f32)
    return (mn + (mx - mn) * (pos.astype(f32) / den)).astype(f32)


def case_index(vol, thr):
    """Per cell [nx-1, ny-1, nz-1]: bit c = x + 2y + 4z set when that corner is inside."""
    ins = inside_mask(vol, thr)
    nx, ny, nz = vol.shape
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        x, y, z = c & 1, c >> 1 & 1, c >> 2 & 1
        case |= ins[x:x + nx - 1, y:y + ny - 1, z:z + nz - 1].astype(np.int64) << c
    return case


def edge_owner(shape, cell_p, edge):
    """The lattice point and axis that own cell edge `edge` of the cell at cell_p."""
    nx, ny, nz = shape
    base = gen.EDGE_BASE[edge]
    return cell_p + (base & 1) * ny * nz + (base >> 1 & 1) * nz + (base >> 2 & 1), edge // 4


# ---- the table walker (CPU restatement of the whole extraction) -------------

def walk(vol, thr):
    """-> vertices f32 [V,3] in lattice units (by (p, axis)), faces int64 [T,3]
    (by cell, table order)."""
    tab = table()
    shape = vol.shape
    nx, ny, nz = shape
    p, axis, flags = crossed_edges(vol, thr)
    verts = vertex_rule(vol, thr, p, axis)
    vid = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(p, axis))}
    case = case_index(vol, thr)
    faces = []
    for i, j, k in zip(*np.nonzero((case != 0) & (case != 255))):
        cell_p = (int(i) * ny + int(j)) * nz + int(k)
        for tri in tab[case[i, j, k]]:
            faces.append([vid[edge_owner(shape, cell_p, e)] for e in tri])
    return verts, np.array(faces, np.int64).reshape(-1, 3)


# ---- mesh properties ----------------------------------------------------------

def half_edge_counts(faces, V):
    f = np.asarray(faces, np.int64)
    he = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(he[:, 0] * V + he[:, 1], return_counts=True)


def assert_closed_manifold(faces, V):
    """Every directed half-edge occurs exactly once and its reverse exactly once."""
    keys, counts = half_edge_counts(faces, V)
    assert counts.max() == 1, "a directed edge is used twice"
    rev = (keys % V) * V + keys // V
    assert np.array_equal(np.sort(rev), keys), "an edge has no opposite"


def euler(faces, V_used=None):
    f = np.asarray(faces, np.int64)
    used = np.unique(f)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    return len(used) - len(e) + len(f)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def area(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)
