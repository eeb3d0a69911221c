"""Mesh preparation and the SDF batch (the reference's sdf/provider.py).

The reference loads the mesh with trimesh, draws 2^18 points per step from it
on the host and signs the second half with pysdf (provider.py:28-88). Here the
mesh is prepared once on the host in float64 numpy (prepare_mesh), and every
step's batch is drawn and signed on the device (csrc/sdf.hip: ngp_sdf_sample,
ngp_sdf_query): two launches, no host synchronisation. DESIGN.md §21.
"""
import os
import warnings

import numpy as np
import torch

import _ngp_native as nat

BLOCK_FACES = 64  # include/ngp_hip.h NGP_SDF_BLOCK_FACES


# ---- files ----------------------------------------------------------------------

def read_obj(path):
    """`v` and `f` records of a Wavefront OBJ -> (vertices f64 [V, 3], faces
    int64 [T, 3]). Index forms i, i/j, i/j/k, i//k; a negative index counts back
    from the vertices read so far; a polygon is split as a fan."""
    verts, faces = [], []
    with open(path, "r") as fh:
        for ln in fh:
            tok = ln.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(t) for t in tok[1:4]])
            elif tok[0] == "f":
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    return (np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3))


def read_mesh(path):
    """.ply (nerf.mesh.read_ply) or .obj -> (vertices f64 [V, 3], faces int64 [T, 3])."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".ply":
        from nerf.mesh import read_ply
        v, f, _ = read_ply(path)
        return v.astype(np.float64), f.astype(np.int64)
    if ext == ".obj":
        return read_obj(path)
    raise ValueError(f"{path}: only .obj and .ply meshes are read")


# ---- preparation ------------------------------------------------------------------

def _morton_order(centroids):
    """argsort of the 30-bit Morton code of the centroids in their bounding box (stable)."""
    lo, hi = centroids.min(0), centroids.max(0)
    q = ((centroids - lo) / np.maximum(hi - lo, 1e-300) * 1023.0).astype(np.uint64)
    q = np.minimum(q, np.uint64(1023))

    def spread(x):
        x = (x | (x << np.uint64(16))) & np.uint64(0x030000FF)
        x = (x | (x << np.uint64(8))) & np.uint64(0x0300F00F)
        x = (x | (x << np.uint64(4))) & np.uint64(0x030C30C3)
        x = (x | (x << np.uint64(2))) & np.uint64(0x09249249)
        return x
    code = spread(q[:, 0]) | (spread(q[:, 1]) << np.uint64(1)) | (spread(q[:, 2]) << np.uint64(2))
    return np.argsort(code, kind="stable")


def _edge_keys(faces, V):
    """Per face and edge (ab, bc, ca): the undirected key min * V + max and the direction (+1: min -> max)."""
    a = faces[:, [0, 1, 2]]
    b = faces[:, [1, 2, 0]]
    return np.minimum(a, b) * np.int64(V) + np.maximum(a, b), np.where(a < b, 1, -1)


class MeshSDF:
    """A prepared mesh. Device tensors: tris f32 [T, 9], normals f32 [T, 7, 3]
    (face, edges ab bc ca, vertices a b c), block_aabb f32 [ceil(T / 64), 6],
    cdf f32 [T]. Host: vertices f64 [V, 3] (normalised), faces int64 [T, 3]
    (oriented, in the device order), center, scale, watertight."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def T(self):
        return int(self.tris.shape[0])

    @property
    def device(self):
        return self.tris.device


def prepare_mesh(vertices, faces, device=None):
    """Normalise, validate, orient and order a mesh for ngp_sdf_sample / ngp_sdf_query -> MeshSDF."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = v.shape[0]
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError(f"prepare_mesh: face index outside [0, {V})")
    if V == 0 or not np.all(np.isfinite(v)):
        raise ValueError("prepare_mesh: no vertices, or vertices that are not finite")
    # the reference's normalisation (sdf/provider.py:37-43)
    vmin, vmax = v.min(0), v.max(0)
    center = (vmin + vmax) / 2
    scale = 2 / np.sqrt(np.sum((vmax - vmin) ** 2)) * 0.95
    v = (v - center[None, :]) * scale

    def corners(ff):
        return v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]]
    a, b, c = corners(f)
    cr = np.cross(b - a, c - a)
    edge2 = np.maximum(np.maximum(((b - a) ** 2).sum(1), ((c - a) ** 2).sum(1)), ((c - b) ** 2).sum(1))
    keep = np.sqrt((cr ** 2).sum(1)) > 1e-12 * edge2
    if not keep.all():
        warnings.warn(f"prepare_mesh: dropped {int((~keep).sum())} zero-area face(s)")
        f = f[keep]
    if f.shape[0] == 0:
        raise ValueError("prepare_mesh: no face with an area is left")
    a, b, c = corners(f)
    if np.einsum("ij,ij->i", a, np.cross(b, c)).sum() < 0:  # six times the signed volume
        f = f[:, [0, 2, 1]]
    key, direction = _edge_keys(f, V)
    uniq, inv, counts = np.unique(key.reshape(-1), return_inverse=True, return_counts=True)
    balance = np.zeros(uniq.size, np.int64)
    np.add.at(balance, inv, direction.reshape(-1))
    watertight = bool(np.all(counts == 2) and np.all(balance == 0))
    if not watertight:
        print("[WARN] mesh is not watertight! SDF maybe incorrect.")

    a, b, c = corners(f)
    f = f[_morton_order((a + b + c) / 3)]
    a, b, c = corners(f)
    T = f.shape[0]
    cr = np.cross(b - a, c - a)
    area2 = np.sqrt((cr ** 2).sum(1))
    nrm = cr / area2[:, None]
    # edges: the sum of the incident faces' normals, by sorted vertex pair
    key, _ = _edge_keys(f, V)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    esum = np.zeros((uniq.size, 3))
    np.add.at(esum, inv, np.repeat(nrm, 3, axis=0))
    edge_n = esum[inv].reshape(T, 3, 3)
    # vertices: angle-weighted (Baerentzen and Aanaes)
    P = np.stack([a, b, c], 1)

    def angle(i):
        e1, e2 = P[:, (i + 1) % 3] - P[:, i], P[:, (i + 2) % 3] - P[:, i]
        cs = np.einsum("ij,ij->i", e1, e2) / np.sqrt((e1 ** 2).sum(1) * (e2 ** 2).sum(1))
        return np.arccos(np.clip(cs, -1.0, 1.0))
    vsum = np.zeros((V, 3))
    for i in range(3):
        np.add.at(vsum, f[:, i], angle(i)[:, None] * nrm)
    normals = np.concatenate([nrm[:, None], edge_n, vsum[f]], 1)  # [T, 7, 3]

    tris32 = P.reshape(T, 9).astype(np.float32)
    nb = (T + BLOCK_FACES - 1) // BLOCK_FACES
    boxes = np.empty((nb, 6), np.float32)
    for k in range(nb):  # of the float32 corners the kernel reads
        blk = tris32[k * BLOCK_FACES:(k + 1) * BLOCK_FACES].reshape(-1, 3)
        boxes[k, :3], boxes[k, 3:] = blk.min(0), blk.max(0)
    cdf = (np.cumsum(area2) / area2.sum()).astype(np.float32)
    cdf[-1] = 1.0

    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    dev = torch.device(device)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    return MeshSDF(tris=up(tris32), normals=up(normals.astype(np.float32)), block_aabb=up(boxes), cdf=up(cdf),
                   vertices=v, faces=f, center=center, scale=float(scale), watertight=watertight)


# ---- the kernels --------------------------------------------------------------------

def new_counter(device, step=0):
    """ngp_sdf_sample's counter: int32 [2] = (step, the launch's ticket)."""
    return torch.tensor([int(step), 0], dtype=torch.int32, device=device)


def sdf_sample(mesh, N, seed, counter, points=None, tri=None, with_tri=True):
    """One batch (ngp_sdf_sample) -> (points f32 [N, 3], tri int32 [N] or None); counter[0] advances by 1."""
    dev = mesh.device
    nat.check_tensor(mesh.tris, "mesh.tris", dtypes=(torch.float32,), what="float32")
    nat.check_tensor(counter, "counter", dtypes=(torch.int32,), what="int32")
    if counter.numel() != 2:
        raise RuntimeError("counter must hold two int32")
    N = int(N)
    if points is None:
        points = torch.empty(N, 3, device=dev)
    if tri is None and with_tri:
        tri = torch.empty(N, dtype=torch.int32, device=dev)
    P = nat.ptr
    nat.check(nat.lib().ngp_sdf_sample(P(mesh.tris), P(mesh.cdf), mesh.T, N, int(seed) & 0xFFFFFFFF, P(counter),
                                       P(points), P(tri), nat.stream_of(mesh.tris)), "sdf_sample")
    return points, tri


def sdf_query(mesh, points, tri=None, cull=True, feature=False, out=None):
    """Exact signed distance of points f32 [n, 3] to the mesh, negative inside
    (ngp_sdf_query) -> sdf f32 [n], or (sdf, feature int32 [n])."""
    nat.check_tensor(points, "points", dtypes=(torch.float32,), what="float32")
    nat.check_tensor(mesh.tris, "mesh.tris", dtypes=(torch.float32,), what="float32")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("points must be [n, 3]")
    n, dev = int(points.shape[0]), points.device
    if tri is not None:
        nat.check_tensor(tri, "tri", dtypes=(torch.int32,), what="int32")
        if tri.numel() != n:
            raise RuntimeError("tri must hold one entry per point")
    sdf = torch.empty(n, device=dev) if out is None else out
    if out is not None:
        nat.check_tensor(out, "out", dtypes=(torch.float32,), what="float32")
        if out.numel() != n:
            raise RuntimeError("out must hold one entry per point")
    feat = torch.empty(n, dtype=torch.int32, device=dev) if feature else None
    P = nat.ptr
    nat.check(nat.lib().ngp_sdf_query(P(points), n, P(mesh.tris), P(mesh.normals), P(mesh.block_aabb), mesh.T,
                                      P(tri), int(bool(cull)), P(sdf), P(feat), nat.stream_of(points)), "sdf_query")
    return (sdf, feat) if feature else sdf


def morton_perm(points, group=None):
    """A permutation that puts points of [-1, 1]^3 (clamped) in Morton order of
    a 128^3 lattice; with group (bool [n]) the points of the group come last,
    in Morton order among themselves."""
    import raymarching
    q = ((points + 1.0) * 63.5).clamp_(0, 127).int()
    key = raymarching.morton3D(q)
    if group is not None:
        key = key | (group.int() << 21)
    return torch.argsort(key)


# The culled scan is the default of the batch and of the volume; whether the
# batch's points are sorted first is DESIGN.md §21's measured choice.
SORT_POINTS = True


class SDFDataset:
    """SDFDataset (sdf/provider.py:28-88) on the device: sample() -> {"points"
    f32 [N, 3], "sdfs" f32 [N, 1]} in the reference's layout, the first half's
    sdfs 0, the rest ngp_sdf_query's, clipped when clip_sdf is set. The tensors
    are the dataset's own buffers: the next sample() overwrites them. Nothing
    is read back; the step counter lives on the device."""

    def __init__(self, mesh, num_samples=2 ** 18, clip_sdf=None, seed=0, cull=True, sort=None):
        if num_samples % 8 != 0:
            raise ValueError("num_samples must be divisible by 8.")
        if not mesh.tris.is_cuda:
            raise RuntimeError("SDFDataset needs a mesh prepared on a CUDA device (no CPU path exists)")
        self.mesh, self.num_samples, self.clip_sdf, self.seed = mesh, int(num_samples), clip_sdf, int(seed)
        self.cull = bool(cull)
        self.sort = SORT_POINTS if sort is None else bool(sort)
        dev, N = mesh.device, self.num_samples
        self.counter = new_counter(dev)
        self.points = torch.empty(N, 3, device=dev)
        self.tri = torch.empty(N, dtype=torch.int32, device=dev)
        self.sdfs = torch.zeros(N, 1, device=dev)

    def sample(self):
        N, h = self.num_samples, self.num_samples // 2
        sdf_sample(self.mesh, N, self.seed, self.counter, self.points, self.tri)
        pts, tri, out = self.points[h:], self.tri[h:], self.sdfs[h:].view(-1)
        if self.sort and self.cull:
            perm = morton_perm(pts, tri < 0)  # the uniform points, far from the surface, in waves of their own
            out[perm] = sdf_query(self.mesh, pts[perm].contiguous(), tri[perm].contiguous(), cull=True)
        else:
            sdf_query(self.mesh, pts, tri, cull=self.cull, out=out)
        if self.clip_sdf is not None:
            out.clamp_(-self.clip_sdf, self.clip_sdf)
        return {"points": self.points, "sdfs": self.sdfs}


def mesh_sdf_volume(mesh, resolution, chunk=2 ** 20, cull=True):
    """Exact signed distances on the resolution^3 lattice of [-1, 1]^3 -> f32 [R, R, R] (meshgrid 'ij' order)."""
    from nerf.mesh import lattice_points
    R = int(resolution)
    if R < 2:
        raise ValueError("resolution must be at least 2")
    if not mesh.tris.is_cuda:
        raise RuntimeError("mesh_sdf_volume needs a mesh prepared on a CUDA device (no CPU path exists)")
    N, dev = R ** 3, mesh.device
    chunk = max(1, min(int(chunk), N))
    xyzs = torch.empty(chunk, 3, device=dev)
    volume = torch.empty(N, device=dev)
    aabb = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        sdf_query(mesh, lattice_points((R, R, R), aabb, lo, hi, xyzs), cull=cull, out=volume[lo:hi])
    return volume.view(R, R, R)
