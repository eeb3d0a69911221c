"""TensoRF's vector-matrix (VM) decomposition on csrc/tensorf.hip.

A set is three planes and three lines. Component i is a plane over the axes
MAT_IDS[i] (W along the first, H along the second) times a line over the axis
VEC_IDS[i]. Here a plane is stored [H, W, R] and a line [D, R] (one bilinear
corner is R contiguous floats); the reference keeps [1, R, H, W] and
[1, R, D, 1], and plane_to_ref / plane_from_ref / line_to_ref / line_from_ref
convert between the two.

vm_sample is the kernel path (one call for the density set's sum and the
colour set's products); vm_reference is the same quantity through
F.grid_sample on reference-layout tensors, in any dtype, on any device.
DESIGN.md §22."""
import ctypes

import torch
import torch.nn.functional as F
from torch.amp import custom_bwd, custom_fwd

MAT_IDS = ((0, 1), (0, 2), (1, 2))
VEC_IDS = (2, 1, 0)


# ------------------------------------------------------------------ the two layouts
def plane_to_ref(p):
    """[H, W, R] -> [1, R, H, W] (contiguous)."""
    return p.permute(2, 0, 1).unsqueeze(0).contiguous()


def plane_from_ref(p):
    """[1, R, H, W] -> [H, W, R] (contiguous)."""
    return p.squeeze(0).permute(1, 2, 0).contiguous()


def line_to_ref(v):
    """[D, R] -> [1, R, D, 1] (contiguous)."""
    return v.t().unsqueeze(0).unsqueeze(-1).contiguous()


def line_from_ref(v):
    """[1, R, D, 1] -> [D, R] (contiguous)."""
    return v.squeeze(-1).squeeze(0).t().contiguous()


def normalise(x, aabb):
    """World units -> [-1, 1] inside aabb [6]: 2 * (x - lo) / (hi - lo) - 1 in x's dtype."""
    aabb = aabb.to(x.dtype)
    return 2 * (x - aabb[:3]) / (aabb[3:] - aabb[:3]) - 1


def vm_reference(x, planes, lines, mode, aabb=None):
    """The decomposition by definition. x [N, 3] (normalised coordinates, or
    world units with aabb [6]); planes [1, R_i, H, W] and lines [1, R_i, D, 1]
    in the reference's layout. Every plane is sampled at (x[MAT_IDS[i][0]],
    x[MAT_IDS[i][1]]) and every line at (0, x[VEC_IDS[i]]) with bilinear
    interpolation, zero padding and align_corners=True. mode "sum": [N], the
    sum over i and r of plane times line; "concat": [N, sum R_i], the
    products, component-major."""
    if mode not in ("sum", "concat"):
        raise ValueError(f"vm_reference: mode must be 'sum' or 'concat', got {mode!r}")
    if aabb is not None:
        x = normalise(x, aabb)
    N = x.shape[0]
    feats = []
    for i in range(3):
        uv = x[:, list(MAT_IDS[i])].view(1, N, 1, 2)
        w = x[:, VEC_IDS[i]]
        zw = torch.stack((torch.zeros_like(w), w), -1).view(1, N, 1, 2)
        pf = F.grid_sample(planes[i], uv, mode="bilinear", padding_mode="zeros", align_corners=True)
        lf = F.grid_sample(lines[i], zw, mode="bilinear", padding_mode="zeros", align_corners=True)
        feats.append(pf.view(-1, N) * lf.view(-1, N))  # [R_i, N]
    if mode == "sum":
        return sum(f.sum(0) for f in feats)
    return torch.cat(feats, 0).t()


# ------------------------------------------------------------------------ kernel path
def _resolution(planes, lines):
    """The three axis lengths of a set in the parameter layout, checked for consistency."""
    res = [None, None, None]

    def put(axis, n, what):
        if res[axis] is None:
            res[axis] = int(n)
        elif res[axis] != int(n):
            raise RuntimeError(f"vm: {what} has {int(n)} texels along axis {axis}, another tensor has {res[axis]}")

    for i in range(3):
        p, v = planes[i], lines[i]
        if p.dim() != 3 or v.dim() != 2 or p.shape[2] != v.shape[1]:
            raise RuntimeError(f"vm: component {i} needs a plane [H, W, R] and a line [D, R], got "
                               f"{list(p.shape)} and {list(v.shape)}")
        put(MAT_IDS[i][0], p.shape[1], f"plane {i}")
        put(MAT_IDS[i][1], p.shape[0], f"plane {i}")
        put(VEC_IDS[i], v.shape[0], f"line {i}")
    return res


def _check(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"vm: {name} must be a contiguous float32 CUDA tensor")


def _vm_set(nat, planes, lines):
    s = nat.VMSet()
    for i in range(3):
        s.plane[i], s.line[i], s.rank[i] = planes[i].data_ptr(), lines[i].data_ptr(), int(planes[i].shape[2])
    return s


class _VM(torch.autograd.Function):
    """(x, aabb, has_sum, has_cat, *tensors) -> (sigma_feat | None, prod | None);
    tensors: per set present, three planes then three lines."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, aabb, has_sum, has_cat, *tensors):
        import _ngp_native as nat
        x, aabb = x.contiguous(), aabb.contiguous()
        _check(x, "x")
        _check(aabb, "aabb")
        if x.dim() != 2 or x.shape[1] != 3 or aabb.numel() != 6:
            raise RuntimeError(f"vm: x must be [N, 3] and aabb [6], got {list(x.shape)} and {list(aabb.shape)}")
        if len(tensors) != 6 * (int(has_sum) + int(has_cat)) or not tensors:
            raise RuntimeError("vm: six tensors (three planes, three lines) per set")
        for k, t in enumerate(tensors):
            _check(t, f"tensor {k}")
        sets = [tensors[k:k + 6] for k in range(0, len(tensors), 6)]
        res = _resolution(sets[0][:3], sets[0][3:])
        if len(sets) == 2 and _resolution(sets[1][:3], sets[1][3:]) != res:
            raise RuntimeError("vm: the two sets have different resolutions")
        N = x.shape[0]
        s_sum = _vm_set(nat, sets[0][:3], sets[0][3:]) if has_sum else None
        cat = sets[-1] if has_cat else None
        s_cat = _vm_set(nat, cat[:3], cat[3:]) if has_cat else None
        sigma = torch.empty(N, device=x.device) if has_sum else None
        prod = torch.empty(N, sum(int(p.shape[2]) for p in cat[:3]), device=x.device) if has_cat else None
        nat.check(nat.lib().ngp_vm_forward(
            nat.ptr(x), N, nat.ptr(aabb), res[0], res[1], res[2],
            ctypes.byref(s_sum) if has_sum else None, nat.ptr(sigma),
            ctypes.byref(s_cat) if has_cat else None, nat.ptr(prod), nat.stream_of(x)), "vm_forward")
        ctx.save_for_backward(x, aabb, *tensors)
        ctx.has_sum, ctx.has_cat, ctx.res = bool(has_sum), bool(has_cat), res
        ctx.set_materialize_grads(False)
        return sigma, prod

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, g_sigma, g_prod):
        import _ngp_native as nat
        if ctx.needs_input_grad[0]:
            raise RuntimeError("vm: there is no gradient with respect to x (the reference never asks for one)")
        x, aabb, *tensors = ctx.saved_tensors
        res, N = ctx.res, x.shape[0]
        sets = [tensors[k:k + 6] for k in range(0, len(tensors), 6)]
        s_sum = _vm_set(nat, sets[0][:3], sets[0][3:]) if ctx.has_sum else None
        s_cat = _vm_set(nat, sets[-1][:3], sets[-1][3:]) if ctx.has_cat else None
        p_sum = ctypes.byref(s_sum) if ctx.has_sum else None
        p_cat = ctypes.byref(s_cat) if ctx.has_cat else None
        g_sigma = None if g_sigma is None else g_sigma.float().contiguous()
        g_prod = None if g_prod is None else g_prod.float().contiguous()
        lib = nat.lib()
        total = lib.ngp_vm_grad_values(res[0], res[1], res[2], p_sum, p_cat)
        nbytes = lib.ngp_vm_backward_scratch_bytes(res[0], res[1], res[2], p_sum, p_cat)
        if total != sum(t.numel() for t in tensors) or nbytes == 0:
            raise RuntimeError(f"vm_backward: {lib.ngp_last_error().decode(errors='replace')}")
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=x.device)
        grads = torch.empty(total, device=x.device)
        nat.check(lib.ngp_vm_backward(nat.ptr(x), N, nat.ptr(aabb), res[0], res[1], res[2], p_sum, nat.ptr(g_sigma),
                                      p_cat, nat.ptr(g_prod), nat.ptr(scratch), nbytes, nat.ptr(grads),
                                      nat.stream_of(x)), "vm_backward")
        out, at = [], 0
        for k, t in enumerate(tensors):
            g = grads[at:at + t.numel()].view(t.shape)
            at += t.numel()
            out.append(g if ctx.needs_input_grad[4 + k] else None)
        return (None, None, None, None, *out)


def vm_sample(x, aabb, sigma=None, color=None):
    """x [N, 3] in world units, aabb [6] -> (sigma_feat [N] | None, prod
    [N, sum R] | None). sigma, color: (planes, lines) in the parameter layout
    ([H, W, R] and [D, R]); sigma is summed over components and ranks, color
    gives the products, component-major. float32 under autocast. The backward
    gives the gradients of every plane and line, none of x."""
    if sigma is None and color is None:
        raise ValueError("vm_sample: no set")
    tensors = []
    for s in (sigma, color):
        if s is not None:
            tensors += list(s[0]) + list(s[1])
    return _VM.apply(x, aabb, sigma is not None, color is not None, *tensors)


def vm_quantum(*grads):
    """The backward's quantum for these output gradients: 2^-32 of the smallest
    power of two above the largest |g| (0 when every gradient is zero)."""
    import math
    m = max(float(g.detach().abs().max()) for g in grads if g is not None and g.numel())
    if m == 0:
        return 0.0
    e = math.frexp(m)[1]  # m = f * 2^e, 0.5 <= f < 1: 2^e > m
    return 2.0 ** (max(e, -125) - 32)
