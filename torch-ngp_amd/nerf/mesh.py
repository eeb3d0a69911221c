"""Mesh export: a triangle mesh of the trained density field.

The reference's Trainer.save_mesh (nerf/utils.py:688-708) queries
model.density() in 128^3 chunks, copies every chunk to the host
(extract_fields, :172-187), runs PyMCubes on the numpy volume (:190-202) and
writes the result with trimesh. Here the lattice is sampled with the density
update's fused query and marching cubes runs on the device (csrc/mesh.hip);
the one host read of an extraction is the vertex and triangle counts, 16 bytes,
because the outputs have to be allocated. DESIGN.md §11 has the conventions.

  * The volume is [nx, ny, nz] float32, meshgrid(x, y, z, 'ij') order; a point
    is inside when value >= threshold (NaN: outside).
  * Vertices come ordered by (lattice point, axis), triangles by (cell, case
    table order), normals pointing from inside to outside; two runs give the
    same bytes.
  * A surface that leaves the sampled box is left open at the border, as
    PyMCubes leaves it.
  * A neighbour value equal to the threshold puts the vertex on that lattice
    point (t = 1). The index structure stays manifold and a few triangles have
    zero area; they are kept.
"""
import ctypes
import os

import numpy as np
import torch

import _ngp_native as nat


def _aabb_list(aabb):
    """aabb (tensor or sequence, min then max) as six Python floats; a device
    tensor is read once here, before any kernel of the extraction is enqueued."""
    if aabb is None:
        return None
    if torch.is_tensor(aabb):
        aabb = aabb.detach().cpu().tolist()
    vals = [float(v) for v in aabb]
    if len(vals) != 6:
        raise RuntimeError("aabb must hold six values: min then max")
    return vals


def _aabb6(aabb):
    vals = _aabb_list(aabb)
    return None if vals is None else (ctypes.c_float * 6)(*vals)


def marching_cubes(volume, threshold, aabb=None, normals=False):
    """volume: float32 CUDA tensor [nx, ny, nz] -> (vertices f32 [V, 3], faces
    int32 [T, 3][, normals f32 [V, 3]]). Without aabb the vertices are in
    lattice units, as mcubes.marching_cubes returns them (utils.py:196); with
    aabb (min then max) they are mapped per axis by min + (max - min) * (v /
    (n - 1)) (:198-201). An empty result returns [0, 3] tensors."""
    nat.check_tensor(volume, "volume", dtypes=(torch.float32,), what="float32")
    if volume.dim() != 3:
        raise RuntimeError("volume must be [nx, ny, nz]")
    nx, ny, nz = (int(s) for s in volume.shape)
    lib, P, dev, s = nat.lib(), nat.ptr, volume.device, nat.stream_of(volume)
    box = _aabb6(aabb)
    ws_bytes = int(lib.ngp_mesh_workspace_bytes(nx, ny, nz))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    nat.check(lib.ngp_mesh_count(P(volume), nx, ny, nz, float(threshold), P(ws), ws_bytes, P(counts), s),
              "mesh_count")
    V, T = (int(c) for c in counts.cpu().tolist())  # the extraction's one host read
    vertices = torch.empty(V, 3, device=dev)
    faces = torch.empty(T, 3, dtype=torch.int32, device=dev)
    nrm = torch.empty(V, 3, device=dev) if normals else None
    if V or T:
        nat.check(lib.ngp_mesh_emit(P(volume), nx, ny, nz, float(threshold), box, P(ws), ws_bytes, V, T,
                                    P(vertices), P(nrm), P(faces), s), "mesh_emit")
    return (vertices, faces, nrm) if normals else (vertices, faces)


def lattice_points(resolution, aabb, lo, hi, out):
    """World positions of lattice points [lo, hi) into out[:hi - lo]."""
    nx, ny, nz = resolution
    nat.check(nat.lib().ngp_mesh_lattice_points(nx, ny, nz, _aabb6(aabb), lo, hi, nat.ptr(out), nat.stream_of(out)),
              "mesh_lattice_points")
    return out[:hi - lo]


def _fused_query(model):
    e, sn = model.encoder, model.sigma_net
    return (getattr(e, "level_dim", None) == 2 and getattr(e, "input_dim", None) == 3
            and getattr(sn, "input_dim", None) == 32 and getattr(sn, "hidden_dim", None) == 64
            and e.num_levels * e.level_dim == 32)


@torch.no_grad()
def sample_density(model, resolution=256, aabb=None, chunk=2 ** 21):
    """The density on a resolution^3 lattice over aabb (default
    model.aabb_infer, as the reference, utils.py:703) -> float32 CUDA volume.
    Chunks of `chunk` points: lattice positions, the fused grid forward on the
    fp16 table copy (NeRFNetwork._query_density's query) and the sigma network
    with its density epilogue, so the encoding buffer stays at chunk * 64
    bytes and nothing visits the host. Models the fused query does not cover
    (level_dim != 2, a sigma network that is not 32 -> 64) take
    model.density() under autocast on the same lattice, chunked too. The value
    is density()'s sigma, without density_scale, as the reference meshes it."""
    res = (int(resolution),) * 3
    N = res[0] ** 3
    aabb = _aabb_list(model.aabb_infer if aabb is None else aabb)
    dev = model.aabb_infer.device
    chunk = max(1, min(int(chunk), N))
    xyzs = torch.empty(chunk, 3, device=dev)
    volume = torch.empty(N, device=dev)
    fused = _fused_query(model)
    if fused:
        lib, P, s = nat.lib(), nat.ptr, nat.stream_of(xyzs)
        e, sn = model.encoder, model.sigma_net
        emb = e.embeddings.detach().half()  # autocast's cast of the table (gridencoder/grid.py)
        w = sn.weights.detach().half().reshape(-1)
        img = torch.empty(int(lib.ngp_ffmlp_image_bytes(sn.input_dim, sn.hidden_dim, sn.num_layers)),
                          dtype=torch.uint8, device=dev)
        nat.check(lib.ngp_ffmlp_pack(1, (ctypes.c_void_p * 1)(P(w)), (ctypes.c_uint32 * 1)(sn.input_dim),
                                     (ctypes.c_uint32 * 1)(sn.hidden_dim), (ctypes.c_uint32 * 1)(sn.num_layers),
                                     (ctypes.c_void_p * 1)(P(img)), s), "ffmlp_pack")
        enc = torch.empty(e.num_levels * chunk * e.level_dim, dtype=torch.float16, device=dev)
        S = float(np.log2(e.per_level_scale))
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        n = hi - lo
        pts = lattice_points(res, aabb, lo, hi, xyzs)
        if fused:
            # encodings [L][n][2] (pair-major, row stride n) at the buffer's head
            nat.check(lib.ngp_grid_encode_forward_fused(
                P(pts), float(model.bound), P(emb), nat.DTYPE_CODE[emb.dtype], P(e.offsets), P(enc), n, None,
                e.input_dim, e.level_dim, e.num_levels, S, e.base_resolution, e.gridtype_id, int(e.align_corners),
                e.interp_id, 0, s), "grid_encode_fused")
            nat.check(lib.ngp_nerf_density_forward_rows(P(enc), P(img), n, sn.hidden_dim, sn.num_layers, 1.0,
                                                        P(volume) + 4 * lo, s), "nerf_density_forward_rows")
        else:
            with torch.autocast("cuda", dtype=torch.float16):
                sigma = model.density(pts)["sigma"]
            volume[lo:hi] = sigma.reshape(-1).float()
    return volume.view(*res)


def extract_geometry(model, resolution=256, threshold=10, aabb=None, normals=False):
    """extract_geometry (utils.py:190-202) on the device: sample_density, then
    marching_cubes with the vertices in world space."""
    aabb = _aabb_list(model.aabb_infer if aabb is None else aabb)
    volume = sample_density(model, resolution, aabb)
    return marching_cubes(volume, threshold, aabb=aabb, normals=normals)


def save_mesh(model, path, resolution=256, threshold=10, normals=True):
    """Trainer.save_mesh (utils.py:688-708): the mesh of the density field over
    model.aabb_infer as a binary PLY -> (vertex count, triangle count)."""
    out = extract_geometry(model, resolution, threshold, normals=normals)
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    write_ply(path, *[t.cpu().numpy() for t in out])
    return int(out[0].shape[0]), int(out[1].shape[0])


# ---- PLY -----------------------------------------------------------------------

_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, vertices, faces, normals=None):
    """Binary little-endian PLY: float x y z [nx ny nz] per vertex, list uchar
    int vertex_indices per face."""
    v = np.ascontiguousarray(np.asarray(vertices, "<f4").reshape(-1, 3))
    f = np.asarray(faces, "<i4").reshape(-1, 3)
    props = ["x", "y", "z"]
    if normals is not None:
        n = np.asarray(normals, "<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("normals must match vertices")
        v = np.ascontiguousarray(np.concatenate([v, n], 1))
        props += ["nx", "ny", "nz"]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property float {p}" for p in props]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], _FACE_DTYPE)
    rec["n"] = 3
    rec["v"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def read_ply(path):
    """What write_ply writes -> (vertices f32 [V, 3], faces int32 [T, 3],
    normals f32 [V, 3] or None)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = nf = 0
    props = []
    for ln in lines:
        tok = ln.split()
        if tok[:2] == ["element", "vertex"]:
            nv = int(tok[2])
        elif tok[:2] == ["element", "face"]:
            nf = int(tok[2])
        elif tok[:2] == ["property", "float"]:
            props.append(tok[2])
    if props not in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"]):
        raise ValueError(f"{path}: unexpected vertex properties {props}")
    v = np.frombuffer(data, "<f4", nv * len(props), end).reshape(nv, len(props))
    rec = np.frombuffer(data, _FACE_DTYPE, nf, end + v.nbytes)
    if nf and not np.all(rec["n"] == 3):
        raise ValueError(f"{path}: only triangles are supported")
    normals = v[:, 3:].copy() if len(props) == 6 else None
    return v[:, :3].copy(), rec["v"].astype(np.int32).reshape(nf, 3), normals
