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

Off by default, after the extraction and on the device as well
(csrc/mesh_clean.hip; the reference has neither): `components`
and `clean` drop small connected components with the order of what stays
kept, `vertex_colors` asks the model for the colour of every vertex seen along
its normal, and write_ply / read_ply know `red green blue`.
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


def save_mesh(model, path, resolution=256, threshold=10, normals=True, colors=False, min_faces=0,
              keep_largest=False, info=None):
    """Trainer.save_mesh (utils.py:688-708): the mesh of the density field over
    model.aabb_infer as a binary PLY -> (vertex count, triangle count) of what
    was written. min_faces > 0 or keep_largest: the mesh is cleaned first
    (clean; its info dict is copied into `info` when one is given). colors:
    vertex_colors of the vertices that are left, as red green blue. With none
    of the three this issues the calls and writes the bytes it always did."""
    cleaning = int(min_faces) > 0 or bool(keep_largest)
    want_normals = bool(normals) or bool(colors)  # the colour query looks along the normal
    out = extract_geometry(model, resolution, threshold, normals=want_normals)
    verts, faces, nrm = (out + (None,))[:3]
    if cleaning:
        verts, faces, nrm, cinfo = clean(verts, faces, nrm, min_faces=min_faces, keep_largest=keep_largest)
        if info is not None:
            info.update(cinfo)
    rgb = vertex_colors(model, verts, nrm) if colors else None
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    write_ply(path, verts.cpu().numpy(), faces.cpu().numpy(), nrm.cpu().numpy() if normals else None,
              **({"colors": rgb.cpu().numpy()} if colors else {}))
    return int(verts.shape[0]), int(faces.shape[0])


# ---- components and cleaning (csrc/mesh_clean.hip) ---------------

def _check_faces(faces, V):
    nat.check_tensor(faces, "faces", dtypes=(torch.int32,), what="int32")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("faces must be [T, 3]")
    if int(V) < 0:
        raise RuntimeError("V must not be negative")


def components(faces, V):
    """faces: int32 CUDA tensor [T, 3] over V vertices -> (labels int32 [V],
    comp_faces int32 [V]): labels[v] is the smallest vertex index of v's
    connected component (two vertices are connected when a triangle holds
    both), comp_faces[r] the triangle count of the component labelled r and 0
    where r is no label. A face with an index outside [0, V) is ignored.
    Nothing is read back."""
    _check_faces(faces, V)
    V, T, dev = int(V), int(faces.shape[0]), faces.device
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    comp_faces = torch.empty(V, dtype=torch.int32, device=dev)
    nat.check(nat.lib().ngp_mesh_components(nat.ptr(faces), V, T, nat.ptr(labels), nat.ptr(comp_faces),
                                            nat.stream_of(faces)), "mesh_components")
    return labels, comp_faces


def clean(vertices, faces, normals=None, min_faces=0, keep_largest=False):
    """Drop small components: -> (vertices, faces, normals or None, info).
    A component is kept when it has at least min_faces triangles and, with
    keep_largest, is also the one with the most triangles (a tie: the smaller
    label). A triangle stays when its component does (and its indices are
    valid), a vertex when a triangle that stays uses it, so min_faces=1 alone
    drops unreferenced vertices and invalid faces only. What stays keeps its
    order; the faces are re-indexed. info: components, components_kept,
    vertices_dropped, faces_dropped. One host read, 32 bytes, for the sizes."""
    nat.check_tensor(vertices, "vertices", dtypes=(torch.float32,), what="float32")
    V = int(vertices.shape[0])
    _check_faces(faces, V)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("vertices must be [V, 3]")
    if normals is not None:
        nat.check_tensor(normals, "normals", dtypes=(torch.float32,), what="float32")
        if normals.shape != vertices.shape:
            raise RuntimeError("normals must match vertices")
    if int(min_faces) < 0:
        raise RuntimeError("min_faces must not be negative")
    T, dev = int(faces.shape[0]), vertices.device
    lib, P, s = nat.lib(), nat.ptr, nat.stream_of(vertices)
    labels, comp_faces = components(faces, V)
    ws_bytes = int(lib.ngp_mesh_clean_workspace_bytes(V, T))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    nat.check(lib.ngp_mesh_clean_count(P(faces), V, T, P(labels), P(comp_faces), int(min_faces), int(bool(keep_largest)),
                                       P(ws), ws_bytes, P(counts), s), "mesh_clean_count")
    V2, T2, ncomp, nkept = (int(c) for c in counts.cpu().tolist())  # the clean's one host read
    v2 = torch.empty(V2, 3, device=dev)
    f2 = torch.empty(T2, 3, dtype=torch.int32, device=dev)
    n2 = torch.empty(V2, 3, device=dev) if normals is not None else None
    if V2 or T2:
        nat.check(lib.ngp_mesh_clean_emit(P(vertices), P(normals), P(faces), V, T, P(ws), ws_bytes, V2, T2, P(v2),
                                          P(n2), P(f2), s), "mesh_clean_emit")
    info = dict(components=ncomp, components_kept=nkept, vertices_dropped=V - V2, faces_dropped=T - T2)
    return v2, f2, n2, info


# ---- vertex colours ---------------------------------------------------------------

def _fused_color_query(model):
    """ngp_nerf_forward's shapes on top of the fused grid query's: both
    networks 64 wide, 2..3 / 2..4 layers, the colour input [SH4(d) | 15
    geometry features | pad]."""
    sn, cn, ed = model.sigma_net, model.color_net, model.encoder_dir
    return (_fused_query(model) and sn.num_layers in (2, 3) and getattr(sn, "output_dim", None) == 16
            and getattr(cn, "input_dim", None) == 32 and getattr(cn, "hidden_dim", None) == 64
            and cn.num_layers in (2, 3, 4) and getattr(ed, "degree", None) == 4
            and getattr(ed, "input_dim", None) == 3 and getattr(ed, "output_dim", None) == 16)


@torch.no_grad()
def vertex_colors(model, vertices, normals, chunk=2 ** 20):
    """The model's colour at every vertex seen along -normal -> uint8 CUDA
    tensor [V, 3]. d = -n / |n| is the view direction of a camera that looks
    straight at the surface ((0, 0, 1) where the normal is zero or not
    finite). Chunks of `chunk` vertices: the directions, the fused grid
    forward on the fp16 table copy (sample_density's set-up), both networks
    in one launch (ngp_nerf_forward), then sigmoid and the frame renderer's
    quantisation in one kernel; nothing visits the host. Models outside those
    shapes take model(x, d) under autocast on the same chunks and the same
    last kernel."""
    nat.check_tensor(vertices, "vertices", dtypes=(torch.float32,), what="float32")
    nat.check_tensor(normals, "normals", dtypes=(torch.float32,), what="float32")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or normals.shape != vertices.shape:
        raise RuntimeError("vertices and normals must both be [V, 3]")
    V, dev = int(vertices.shape[0]), vertices.device
    rgb = torch.empty(V, 3, dtype=torch.uint8, device=dev)
    if V == 0:
        return rgb
    chunk = max(1, min(int(chunk), V))
    lib, P, s = nat.lib(), nat.ptr, nat.stream_of(vertices)
    dirs = torch.empty(chunk, 3, device=dev)
    fused = _fused_color_query(model)
    if fused:
        e, sn, cn = model.encoder, model.sigma_net, model.color_net
        nets = (sn, cn)
        emb = e.embeddings.detach().half()  # autocast's cast of the table (gridencoder/grid.py)
        w = [n.weights.detach().half().reshape(-1) for n in nets]
        img = [torch.empty(int(lib.ngp_ffmlp_image_bytes(n.input_dim, n.hidden_dim, n.num_layers)),
                           dtype=torch.uint8, device=dev) for n in nets]
        nat.check(lib.ngp_ffmlp_pack(2, (ctypes.c_void_p * 2)(*[P(t) for t in w]),
                                     (ctypes.c_uint32 * 2)(*[n.input_dim for n in nets]),
                                     (ctypes.c_uint32 * 2)(*[n.hidden_dim for n in nets]),
                                     (ctypes.c_uint32 * 2)(*[n.num_layers for n in nets]),
                                     (ctypes.c_void_p * 2)(*[P(t) for t in img]), s), "ffmlp_pack")
        h16 = torch.float16
        enc = torch.empty(e.num_levels * chunk * e.level_dim, dtype=h16, device=dev)
        h_out = torch.empty(chunk, 16, dtype=h16, device=dev)
        sigma = torch.empty(chunk, device=dev)
        color_in = torch.empty(chunk, 32, dtype=h16, device=dev)
        color_out = torch.empty(chunk, 16, dtype=h16, device=dev)
        S = float(np.log2(e.per_level_scale))
    for lo in range(0, V, chunk):
        n = min(lo + chunk, V) - lo
        pts = vertices[lo:lo + n]
        nat.check(lib.ngp_mesh_color_dirs(P(normals) + 12 * lo, n, P(dirs), s), "mesh_color_dirs")
        out = P(rgb) + 3 * lo
        if fused:
            # encodings [L][n][2] (pair-major, row stride n) at the buffer's head
            nat.check(lib.ngp_grid_encode_forward_fused(
                P(pts), float(model.bound), P(emb), nat.DTYPE_CODE[emb.dtype], P(e.offsets), P(enc), n, None,
                e.input_dim, e.level_dim, e.num_levels, S, e.base_resolution, e.gridtype_id, int(e.align_corners),
                e.interp_id, 0, s), "grid_encode_fused")
            nat.check(lib.ngp_nerf_forward(P(enc), P(img[0]), P(img[1]), n, None, sn.hidden_dim, sn.num_layers,
                                           cn.hidden_dim, cn.num_layers, P(h_out), P(sigma), P(color_in), P(dirs),
                                           float(model.density_scale), P(color_out), s), "nerf_forward")
            nat.check(lib.ngp_mesh_color_finish(P(color_out), 16, n, 1, out, s), "mesh_color_finish")
        else:
            with torch.autocast("cuda", dtype=torch.float16):
                c = model(pts, dirs[:n])[1]
            c = c.half().contiguous()  # sigmoid already applied: the kernel only quantises
            nat.check(lib.ngp_mesh_color_finish(P(c), int(c.shape[1]), n, 0, out, s), "mesh_color_finish")
    return rgb


# ---- PLY -----------------------------------------------------------------------

_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
_COLOR_PROPS = ["red", "green", "blue"]


def write_ply(path, vertices, faces, normals=None, colors=None):
    """Binary little-endian PLY: float x y z [nx ny nz] [uchar red green blue]
    per vertex, list uchar int vertex_indices per face. Without colours the
    file is the one this function always wrote."""
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
    if colors is not None:
        c = np.asarray(colors)
        if c.dtype != np.uint8 or c.reshape(-1, 3).shape[0] != v.shape[0]:
            raise ValueError("colors must be uint8 [V, 3]")
        header += [f"property uchar {p}" for p in _COLOR_PROPS]
        # one unpadded record per vertex: 15 or 27 bytes
        packed = np.empty(v.shape[0], np.dtype([("f", "<f4", (len(props),)), ("c", "u1", (3,))]))
        packed["f"] = v
        packed["c"] = c.reshape(-1, 3)
        v = packed
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], _FACE_DTYPE)
    rec["n"] = 3
    rec["v"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def read_ply(path, with_colors=False):
    """What write_ply writes -> (vertices f32 [V, 3], faces int32 [T, 3],
    normals f32 [V, 3] or None); with_colors: a fourth entry, colours uint8
    [V, 3] or None. A coloured file read without with_colors gives the three."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = nf = 0
    props, cprops = [], []
    for ln in lines:
        tok = ln.split()
        if tok[:2] == ["element", "vertex"]:
            nv = int(tok[2])
        elif tok[:2] == ["element", "face"]:
            nf = int(tok[2])
        elif tok[:2] == ["property", "float"]:
            if cprops:
                raise ValueError(f"{path}: a float property after the colours")
            props.append(tok[2])
        elif tok[:2] == ["property", "uchar"]:
            cprops.append(tok[2])
    if props not in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"]):
        raise ValueError(f"{path}: unexpected vertex properties {props}")
    if cprops not in ([], _COLOR_PROPS):
        raise ValueError(f"{path}: unexpected vertex properties {cprops}")
    vrec = np.dtype([("f", "<f4", (len(props),))] + ([("c", "u1", (3,))] if cprops else []))
    vr = np.frombuffer(data, vrec, nv, end)
    v = vr["f"].reshape(nv, len(props))
    rec = np.frombuffer(data, _FACE_DTYPE, nf, end + nv * vrec.itemsize)
    if nf and not np.all(rec["n"] == 3):
        raise ValueError(f"{path}: only triangles are supported")
    normals = v[:, 3:].copy() if len(props) == 6 else None
    out = (v[:, :3].copy(), rec["v"].astype(np.int32).reshape(nf, 3), normals)
    if with_colors:
        out += (vr["c"].reshape(nv, 3).copy() if cprops else None,)
    return out
