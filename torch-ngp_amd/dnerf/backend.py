"""ctypes shims over csrc/dnerf.hip (include/ngp_hip.h): the
deformation network's input row and the time-sliced density grid's update.
There is no fallback: without the library or a GPU every call raises."""
import torch

import _ngp_native as nat

ENCODE_COLS = nat.DNERF_ENCODE_COLS


def encode(x, t, dtype=torch.float32, out=None):
    """[x's frequency encoding (10 octaves), t's (6 octaves)] -> [N, 76].
    x f32 [N, 3]; t f32 [1, 1] (one time for every row) or [N, 1]. out: a
    float or half [N, >= 76] tensor with unit column stride to write into (the
    columns past 76 stay untouched); default a new contiguous tensor of `dtype`."""
    nat.check_tensor(x, "x", (torch.float32,), "float32")
    nat.check_tensor(t, "t", (torch.float32,), "float32")
    N = x.shape[0]
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError(f"dnerf.encode: x must be [N, 3], got {list(x.shape)}")
    if t.numel() == 1:
        t_stride = 0
    elif t.numel() == N:
        t_stride = 1
    else:
        raise RuntimeError(f"dnerf.encode: t must hold 1 or N = {N} values, got {t.numel()}")
    if out is None:
        out = torch.empty(N, ENCODE_COLS, dtype=dtype, device=x.device)
    nat.check_tensor(out, "out", (torch.float32, torch.float16), "float32 or float16", contiguous=False)
    if out.dim() != 2 or out.shape[0] != N or out.shape[1] < ENCODE_COLS or (N > 0 and out.stride(1) != 1) or \
            (N > 1 and out.stride(0) < ENCODE_COLS):
        raise RuntimeError(f"dnerf.encode: out must be [N, >= {ENCODE_COLS}] with unit column stride")
    row_stride = out.stride(0) if N > 1 else max(out.stride(0), ENCODE_COLS)
    nat.check(nat.lib().ngp_dnerf_encode(nat.ptr(x), nat.ptr(t), t_stride, N, nat.ptr(out), nat.DTYPE_CODE[out.dtype],
                                         row_stride, nat.stream_of(x)), "dnerf_encode")
    return out


def grid_points_workspace(T, C, H, device):
    """The occupied-cell lists of a partial update (uint8 tensor)."""
    n = nat.lib().ngp_dnerf_grid_points_workspace_bytes(T, C, H)
    if n == 0:
        raise RuntimeError(f"dnerf.grid_points_workspace: bad grid shape T={T} C={C} H={H}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def grid_points(grid, T, C, H, bound, partial, seed, update, lo, hi, ws=None):
    """Query points [lo, hi) of an update -> xyzs [n, 3], times [n], indices i32 [n]."""
    if grid is not None:
        nat.check_tensor(grid, "grid", (torch.float32,), "float32")
    if ws is not None:
        nat.require_cuda(ws, "ws")
    dev = grid.device if grid is not None else torch.device("cuda", torch.cuda.current_device())
    n = max(int(hi) - int(lo), 0)
    xyzs = torch.empty(n, 3, device=dev)
    times = torch.empty(n, device=dev)
    indices = torch.empty(n, dtype=torch.int32, device=dev)
    nat.check(nat.lib().ngp_dnerf_grid_points(nat.ptr(grid), T, C, H, float(bound), int(bool(partial)),
                                              int(seed) & 0xffffffff, int(update) & 0xffffffff, lo, hi, nat.ptr(ws),
                                              0 if ws is None else ws.numel() * ws.element_size(), nat.ptr(xyzs),
                                              nat.ptr(times), nat.ptr(indices), nat.stream_of(xyzs)),
              "dnerf_grid_points")
    return xyzs, times, indices


def grid_ema_pack(grid, tmp, T, C, H, decay, density_thresh, bitfield, stats=None):
    """The update's EMA, sum and every slice's bitfield -> stats (f64, [0] the sum of clamp(grid, 0))."""
    nat.check_tensor(grid, "grid", (torch.float32,), "float32")
    nat.check_tensor(tmp, "tmp", (torch.float32,), "float32")
    nat.check_tensor(bitfield, "bitfield", (torch.uint8,), "uint8")
    if stats is None:
        stats = torch.empty(nat.DNERF_STATS_LEN, dtype=torch.float64, device=grid.device)
    n = T * C * H ** 3
    if grid.numel() != n or tmp.numel() != n or bitfield.numel() * 8 != n or stats.numel() < nat.DNERF_STATS_LEN:
        raise RuntimeError(f"dnerf.grid_ema_pack: grid / tmp of {n} cells, bitfield of {n // 8} bytes and "
                           f"{nat.DNERF_STATS_LEN} stats expected")
    nat.check(nat.lib().ngp_dnerf_grid_ema_pack(nat.ptr(grid), nat.ptr(tmp), T, C, H, float(decay),
                                                float(density_thresh), nat.ptr(stats), nat.ptr(bitfield),
                                                nat.stream_of(grid)), "dnerf_grid_ema_pack")
    return stats
