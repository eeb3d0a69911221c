"""Inputs and a numpy float64 restatement of TensoRF's vector-matrix sampling
(tensoRF/vm.py, csrc/tensorf.hip): corner indices, weights and zero padding
written out by hand. tests/test_tensorf_cpu.py holds the restatement to
vm_reference (torch's grid_sample) in float64."""
import numpy as np
import torch

MAT_IDS = ((0, 1), (0, 2), (1, 2))
VEC_IDS = (2, 1, 0)

UNIT_BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
SHRUNK_BOX = (-0.75, -0.5, -0.25, 0.5, 1.0, 0.875)  # such as a shrink leaves


def make_set(res, ranks, seed, scale=0.1, integers=False):
    """Three planes [1, R_i, H, W] and three lines [1, R_i, D, 1] in the
    reference's layout, float32 on the CPU: N(0, scale^2), or integers in
    [-3, 3]."""
    g = torch.Generator().manual_seed(seed)

    def draw(*shape):
        if integers:
            return torch.randint(-3, 4, shape, generator=g).float()
        return scale * torch.randn(*shape, generator=g)

    planes = [draw(1, ranks[i], res[m1], res[m0]) for i, (m0, m1) in enumerate(MAT_IDS)]
    lines = [draw(1, ranks[i], res[VEC_IDS[i]], 1) for i in range(3)]
    return planes, lines


def to_param_layout(planes, lines, device=None):
    """Reference layout -> ([H, W, R] planes, [D, R] lines), contiguous."""
    from tensoRF.vm import line_from_ref, plane_from_ref
    return ([plane_from_ref(p).to(device) for p in planes], [line_from_ref(v).to(device) for v in lines])


def normalised_points(res, n=4097, seed=0):
    """n >= 80 points in normalised coordinates, float64 [n, 3]: the eight
    box corners, every lattice node (up to 60), 1 + 1e-6, -1.5 and 2.0 on each
    axis with the others inside, three points outside on every axis, then
    uniform points in [-1.2, 1.2]^3. -> (points, index of the first wholly
    outside point, count of those)."""
    rng = np.random.default_rng(seed)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    axes = [np.linspace(-1.0, 1.0, r) if r > 1 else np.zeros(1) for r in res]
    nodes = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)[:60]
    special = []
    for a in range(3):
        for v in (1.0 + 1e-6, -1.5, 2.0):
            p = np.array([0.3, -0.2, 0.55])
            p[a] = v
            special.append(p)
    outside = np.array([[-3.0, 3.5, -4.0], [3.0, 3.0, 3.0], [-4.0, -3.5, 3.0]])
    head = np.concatenate([corners, nodes, np.array(special), outside])
    first_outside = head.shape[0] - 3
    uniform = rng.uniform(-1.2, 1.2, (n - head.shape[0], 3))
    return np.concatenate([head, uniform]), first_outside, 3


def world_points(c, aabb):
    """Normalised float64 coordinates -> float32 world units inside aabb (exact for the unit box)."""
    aabb = np.asarray(aabb, np.float64)
    return (aabb[:3] + (c + 1.0) / 2.0 * (aabb[3:] - aabb[:3])).astype(np.float32)


def _axis(c, size):
    """One axis of bilinear sampling with align_corners=True and zero padding:
    the two texel indices, their weights, and whether each lies in the texture."""
    f = (c + 1.0) / 2.0 * (size - 1)
    i0 = np.floor(f).astype(np.int64)
    i1 = i0 + 1
    w1 = f - i0
    w0 = 1.0 - w1
    return (i0, i1), (w0, w1), ((i0 >= 0) & (i0 < size), (i1 >= 0) & (i1 < size))


def vm_numpy(x, planes, lines, mode, aabb=None):
    """The decomposition in float64 numpy. x [N, 3] (normalised, or world units
    with aabb); planes / lines in the reference's layout (anything np.asarray
    takes). "sum": [N]; "concat": [N, sum R_i], component-major."""
    x = np.asarray(x, np.float64)
    if aabb is not None:
        aabb = np.asarray(aabb, np.float64)
        x = 2.0 * (x - aabb[:3]) / (aabb[3:] - aabb[:3]) - 1.0
    N = x.shape[0]
    feats = []
    for i in range(3):
        P = np.asarray(planes[i], np.float64)[0]        # [R, H, W]
        L = np.asarray(lines[i], np.float64)[0, :, :, 0]  # [R, D]
        R, H, W = P.shape
        D = L.shape[1]
        (x0, x1), (wx0, wx1), (vx0, vx1) = _axis(x[:, MAT_IDS[i][0]], W)
        (y0, y1), (wy0, wy1), (vy0, vy1) = _axis(x[:, MAT_IDS[i][1]], H)
        (z0, z1), (wz0, wz1), (vz0, vz1) = _axis(x[:, VEC_IDS[i]], D)
        p = np.zeros((R, N))
        for yi, wy, vy in ((y0, wy0, vy0), (y1, wy1, vy1)):
            for xi, wx, vx in ((x0, wx0, vx0), (x1, wx1, vx1)):
                ok = vy & vx
                texel = P[:, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]  # [R, N]
                p += np.where(ok, texel * (wx * wy), 0.0)
        l = np.zeros((R, N))
        for zi, wz, vz in ((z0, wz0, vz0), (z1, wz1, vz1)):
            l += np.where(vz, L[:, np.clip(zi, 0, D - 1)] * wz, 0.0)
        feats.append(p * l)
    if mode == "sum":
        return sum(f.sum(0) for f in feats)
    return np.concatenate(feats, 0).T


def reference_error(x32, planes, lines, mode, aabb):
    """max |vm_reference in float32 - vm_reference in float64| on the CPU, on
    the same float32 inputs: the base of every tolerance. -> (error, the
    float64 values)."""
    from tensoRF.vm import vm_reference
    x = torch.as_tensor(x32)
    box = torch.tensor(aabb, dtype=torch.float32)
    ref32 = vm_reference(x, planes, lines, mode, aabb=box)
    ref64 = vm_reference(x.double(), [p.double() for p in planes], [v.double() for v in lines], mode,
                         aabb=box.double())
    return float((ref32.double() - ref64).abs().max()), ref64
