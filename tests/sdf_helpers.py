"""Meshes built in code and numpy references for the SDF family (sdf/,
csrc/sdf.hip): a float64 brute-force signed distance by the pseudo-normal rule
(Baerentzen and Aanaes), the generalised winding number (Van Oosterom and
Strackee), a float32 restatement of the query's arithmetic and one of the
sampler's, written from include/ngp_hip.h."""
import numpy as np

from error_map_helpers import rng_u32, rng_unit


# ---- meshes -----------------------------------------------------------------------

def _outward(v, f):
    """Flip every face when the signed volume is negative."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return (v, f[:, [0, 2, 1]]) if np.einsum("ij,ij->i", a, np.cross(b, c)).sum() < 0 else (v, f)


def _convex(v, f):
    """Orient every face of a convex mesh around the origin outwards."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64).copy()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), a + b + c) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v, f


def tetrahedron():
    return _convex([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])


def cube(offset=(0.0, 0.0, 0.0)):
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    q = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    f = [t for a, b, c, d in q for t in ([a, b, c], [a, c, d])]
    v, f = _convex(v, f)
    return v + np.asarray(offset, np.float64), f


def icosahedron():
    g = (1 + 5 ** 0.5) / 2
    v = [[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
         [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
         [8, 6, 7], [9, 8, 1]]
    return _convex(v, f)


def bipyramid(k=33):
    """Two apexes over a regular k-gon: 2 k faces (66: one full block of 64 and a tail of 2)."""
    t = 2 * np.pi * np.arange(k) / k
    v = np.concatenate([np.stack([np.cos(t), np.sin(t), np.zeros(k)], 1), [[0, 0, 0.8], [0, 0, -0.6]]])
    f = [[k, i, (i + 1) % k] for i in range(k)] + [[k + 1, (i + 1) % k, i] for i in range(k)]
    return _convex(v, f)


def torus(nu=8, nv=6, R=1.0, r=0.4):
    """nu x nv quads split in two: 2 nu nv faces (8 x 6: 96, 32 x 16: 1,024). Non-convex, genus 1."""
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    U, W = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [[a, b, c], [a, c, d]]
    return _outward(v, f)


def two_cubes():
    v1, f1 = cube((-1.6, 0.0, 0.0))
    v2, f2 = cube((1.6, 0.3, -0.2))
    return np.concatenate([v1, v2]), np.concatenate([f1, f2 + 8])


MESHES = {"tetrahedron": tetrahedron, "cube": cube, "icosahedron": icosahedron, "bipyramid_66": bipyramid,
          "torus_96": torus, "torus_1024": lambda: torus(32, 16), "two_cubes": two_cubes}
FACES = {"tetrahedron": 4, "cube": 12, "icosahedron": 20, "bipyramid_66": 66, "torus_96": 96, "torus_1024": 1024,
         "two_cubes": 24}


def write_obj(path, v, f):
    with open(path, "w") as fh:
        for p in v:
            fh.write("v %.17g %.17g %.17g\n" % tuple(p))
        for t in f:
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


# ---- the closest point of a triangle (Ericson 5.1.5), in one dtype ----------------

def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def closest(p, tris, dtype):
    """p [n, 3], tris [T, 3, 3] -> (dist2 [n, T], diff = p - q [n, T, 3], code
    [n, T]): every operation in `dtype` and in the order of csrc/sdf.hip's
    closest(). Codes: 0 face, 1 2 3 edges ab bc ca, 4 5 6 vertices a b c.
    Vectors are kept as three [n, T] component arrays (contiguous operands)."""
    p = np.asarray(p, dtype)
    t = np.asarray(tris, dtype)
    P = [np.ascontiguousarray(p[:, k])[:, None] for k in range(3)]
    a, b, c = ([np.ascontiguousarray(t[:, i, k])[None, :] for k in range(3)] for i in range(3))
    sub = lambda x, y: [x[k] - y[k] for k in range(3)]  # noqa: E731
    ab, ac, bc = sub(b, a), sub(c, a), sub(c, b)
    ap, bp, cp = sub(P, a), sub(P, b), sub(P, c)
    d1, d2 = _dot3(ab, ap), _dot3(ac, ap)
    d3, d4 = _dot3(ab, bp), _dot3(ac, bp)
    d5, d6 = _dot3(ab, cp), _dot3(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    conds = [((d1 <= 0) & (d2 <= 0), 4), ((d3 >= 0) & (d4 <= d3), 5), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1),
             ((d6 >= 0) & (d5 <= d6), 6), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 3),
             ((va <= 0) & (e43 >= 0) & (e56 >= 0), 2)]
    code = np.zeros(d1.shape, np.int32)
    for cond, k in reversed(conds):
        code[cond] = k
    c0, c1, c2, c3 = code == 0, code == 1, code == 2, code == 3
    one, zero = dtype(1), dtype(0)
    den = np.where(c1, d1 - d3, np.where(c3, d2 - d6, np.where(c2, e43 + e56, np.where(c0, (va + vb) + vc, one))))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = one / den
        t1 = np.where(c1, d1 * r, np.where(c0, vb * r, zero))
        t2 = np.where(c3, d2 * r, np.where(c2, e43 * r, np.where(c0, vc * r, zero)))
        from_b, from_c = (code == 5) | c2, code == 6
        diff = [(np.where(from_b, bp[k], np.where(from_c, cp[k], ap[k])) - t1 * ab[k]) - t2 * np.where(c2, bc[k], ac[k])
                for k in range(3)]
    assert diff[0].dtype == dtype
    return _dot3(diff, diff), np.stack(diff, -1), code


_PN = {}


def pseudo_normals(v, f):
    """[T, 7, 3] float64: unit face normal, edge (ab, bc, ca) and vertex (a, b, c) pseudo-normals."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    key = (v.tobytes(), f.tobytes())
    if key not in _PN:
        _PN[key] = _pseudo_normals(v, f)
    return _PN[key]


def _pseudo_normals(v, f):
    P = v[f]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    edge, vert = {}, np.zeros_like(v)
    for t in range(f.shape[0]):
        for k in range(3):
            i, j = int(f[t, k]), int(f[t, (k + 1) % 3])
            edge[(min(i, j), max(i, j))] = edge.get((min(i, j), max(i, j)), 0) + n[t]
            e1, e2 = P[t, (k + 1) % 3] - P[t, k], P[t, (k + 2) % 3] - P[t, k]
            cs = e1 @ e2 / (np.linalg.norm(e1) * np.linalg.norm(e2))
            vert[i] += np.arccos(np.clip(cs, -1, 1)) * n[t]
    out = np.empty((f.shape[0], 7, 3))
    for t in range(f.shape[0]):
        out[t, 0] = n[t]
        for k in range(3):
            i, j = int(f[t, k]), int(f[t, (k + 1) % 3])
            out[t, 1 + k] = edge[(min(i, j), max(i, j))]
            out[t, 4 + k] = vert[i]
    return out


def signed_distance(v, f, points, dtype=np.float64, chunk=128):
    """Brute force over all faces -> (sdf, face, code), negative inside. dtype
    float64: the reference; float32: the kernel's arithmetic (the first face of
    the smallest squared distance, the float32 pseudo-normals prepare_mesh uploads)."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    tris = v[f].astype(dtype)
    pn = pseudo_normals(v, f).astype(dtype)
    points = np.asarray(points, dtype)
    sd, face, code = (np.empty(len(points), dtype), np.empty(len(points), np.int64), np.empty(len(points), np.int64))
    for lo in range(0, len(points), chunk):
        p = points[lo:lo + chunk]
        d2, diff, cd = closest(p, tris, dtype)
        k = np.argmin(d2, axis=1)  # the first of equal minima
        r = np.arange(len(p))
        s = _dot(diff[r, k], pn[k, cd[r, k]])
        d = np.sqrt(d2[r, k])
        sd[lo:lo + chunk] = np.where(s < 0, -d, d)
        face[lo:lo + chunk], code[lo:lo + chunk] = k, cd[r, k]
    return sd, face, code


def winding_number(v, f, points):
    """Generalised winding number: the sum of the faces' solid angles over 4 pi (1 inside a closed outward mesh)."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    out = np.empty(len(points))
    for lo in range(0, len(points), 512):
        p = np.asarray(points[lo:lo + 512], np.float64)[:, None, None, :]
        t = v[f][None] - p
        a, b, c = t[:, :, 0], t[:, :, 1], t[:, :, 2]
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        num = np.einsum("ntk,ntk->nt", a, np.cross(b, c))
        den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
        out[lo:lo + 512] = (2 * np.arctan2(num, den)).sum(1) / (4 * np.pi)
    return out


def box_sdf(points, half=1.0):
    q = np.abs(np.asarray(points, np.float64)) - half
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)


def make_points(v, f, n_uniform, n_near, seed, sigma=0.01, extent=None):
    """Uniform points in the bounding cube (times 1.1) and points sigma * normal
    noise away from random vertices, edge midpoints and face points."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    rng = np.random.default_rng(seed)
    ext = 1.1 * np.abs(v).max() if extent is None else extent
    uni = rng.uniform(-ext, ext, (n_uniform, 3))
    k = n_near // 3
    vert = v[rng.integers(0, len(v), k)]
    t = f[rng.integers(0, len(f), k)]
    e = rng.integers(0, 3, k)
    mid = (v[t[np.arange(k), e]] + v[t[np.arange(k), (e + 1) % 3]]) / 2
    t = f[rng.integers(0, len(f), n_near - 2 * k)]
    w = rng.dirichlet([1, 1, 1], len(t))
    face = np.einsum("nk,nkj->nj", w, v[t])
    near = np.concatenate([vert, mid, face])
    return np.concatenate([uni, near + sigma * rng.standard_normal(near.shape)])


# The distance bound of the query tests: 4 x the largest |d32 - d64| of the
# float32 restatement (signed_distance(dtype=float32)) against the float64
# reference on query_points() of every mesh above, the 4 for libm and ordering
# differences on the device. Measured (tests/test_sdf_cpu.py
# test_restatement_bound): 1.018e-7 on the 66-face bipyramid, the largest.
DIST_BOUND = 4 * 1.02e-7


def query_points(v, f, n=1000, seed=11):
    """The query tests' points on a normalised mesh, float32: a quarter uniform
    in [-1, 1]^3, the rest 0.01 * normal noise from the surface, shuffled."""
    pts = make_points(v, f, n // 4, n - n // 4, seed=seed, extent=1.0)
    return pts[np.random.default_rng(seed).permutation(n)].astype(np.float32)


# ---- the sampler (ngp_sdf_sample) in float32 ------------------------------------------

def sample_f32(tris32, cdf32, N, seed, step):
    """-> (points f32 [N, 3], tri int32 [N]) of step `step`, from include/ngp_hip.h's description."""
    f32 = np.float32
    tris32, cdf32 = np.asarray(tris32, f32).reshape(-1, 3, 3), np.asarray(cdf32, f32)
    T, n = len(cdf32), np.arange(N, dtype=np.uint64)
    u = [rng_unit(seed, step, n, s) for s in range(3)]
    tri = np.minimum(np.searchsorted(cdf32, u[0], side="right"), T - 1).astype(np.int32)
    su = np.sqrt(u[1])
    b0, b1, b2 = f32(1) - su, su * (f32(1) - u[2]), su * u[2]
    a, b, c = tris32[tri, 0], tris32[tri, 1], tris32[tri, 2]
    pts = (b0[:, None] * a + b1[:, None] * b) + b2[:, None] * c
    inv = f32(1.0 / 16777216.0)
    ua = ((rng_u32(seed, step, n, 3) >> np.uint64(8)) + np.uint64(1)).astype(f32) * inv
    uc = ((rng_u32(seed, step, n, 5) >> np.uint64(8)) + np.uint64(1)).astype(f32) * inv
    ub, ud = rng_unit(seed, step, n, 4), rng_unit(seed, step, n, 6)
    ra, rc = np.sqrt(f32(-2) * np.log(ua)), np.sqrt(f32(-2) * np.log(uc))
    pa, pc = f32(6.2831855) * ub, f32(6.2831855) * ud
    z = np.stack([ra * np.cos(pa), ra * np.sin(pa), rc * np.cos(pc)], 1)
    assert pts.dtype == f32 and z.dtype == f32
    noisy = pts + f32(0.01) * z
    uni = np.stack([x * f32(2) - f32(1) for x in u], 1)
    i = np.arange(N)[:, None]
    out = np.where(i < N // 2, pts, np.where(i < N // 8 * 7, noisy, uni)).astype(f32)
    return out, np.where(np.arange(N) < N // 8 * 7, tri, -1).astype(np.int32)
