"""Shared by the SSIM tests (test_ssim_cpu.py, test_gpu_ssim.py; DESIGN.md
section 18): the kernel's tile constants and the shapes they make critical,
made-up inputs (the render's buffers and a 3-view image stack in each store),
the float32 oracle inputs formed as tests/test_gpu_validate.py forms the
squared error's, and a direct 121-tap restatement of the windowed means."""
import numpy as np
import torch

TILE_W, TILE_H = 32, 16  # csrc/frame.hip kSsimTileW, kSsimTileH: output positions per workgroup tile
HALO = 10
C1, C2 = 0.01 * 0.01, 0.03 * 0.03

# (H, W): one position; one extra column; one extra row; odd sizes with partial tiles in both axes;
# exactly one tile of positions; the tile size + 1 positions in both axes (four tiles, three of them slivers)
SHAPES = [(11, 11), (11, 12), (12, 11), (37, 53), (TILE_H + HALO, TILE_W + HALO),
          (TILE_H + 1 + HALO, TILE_W + 1 + HALO)]
STORES = ["rgba8", "rgb8", "rgba32"]
KINDS = ["flat", "noise", "smooth"]
VIEW, N_VIEWS = 1, 3  # not the first image of the stack: the pose's offset into it


def smooth(H, W, phase):
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([0.5 + 0.4 * np.sin(0.21 * r + 0.13 * c * (j + 1) + phase + j) for j in range(3)], -1)


def make_pixels(kind, H, W, store, seed):
    """The image stack [N_VIEWS, H, W, 3 | 4] (CPU tensor) of one store.
    flat: nearly constant and bright (uint8: 255; float32: 0.999, opaque);
    noise: random bytes / values, random alpha; smooth: a sine pattern."""
    rng = np.random.default_rng(seed)
    ch = 3 if store == "rgb8" else 4
    if kind == "flat":
        f = np.full((N_VIEWS, H, W, ch), 0.999 if store == "rgba32" else 1.0)
        if ch == 4:
            f[..., 3] = 1.0
    elif kind == "noise":
        f = rng.random((N_VIEWS, H, W, ch))
    else:
        f = np.stack([np.concatenate([smooth(H, W, 0.7 * v), np.full((H, W, 1), 0.5) + 0.5 * rng.random((H, W, 1))],
                                     -1)[..., :ch] for v in range(N_VIEWS)])
    if store == "rgba32":
        return torch.from_numpy(f.astype(np.float32)).contiguous()
    return torch.from_numpy(np.round(f * 255).astype(np.uint8)).contiguous()


def ground_truth_np(pixels_view):
    """[H, W, 3 | 4] of a stack -> float32 [H, W, 3] as nerf.eval.ground_truth
    gives it (uint8 / 255, RGBA blended on white), in numpy float32."""
    px = pixels_view.numpy()
    px = px.astype(np.float32) / np.float32(255) if px.dtype == np.uint8 else px.astype(np.float32)
    if px.shape[-1] == 4:
        return px[..., :3] * px[..., 3:] + (np.float32(1) - px[..., 3:])
    return px


def make_render(kind, H, W, bg, y, seed):
    """image [H * W, 3] and weights_sum [H * W] (CPU float32 tensors) whose
    blend on `bg` is, up to float32 rounding: flat, the ground truth y plus a
    1e-3 perturbation (the cancellation case); noise, normal noise (negative
    values among them); smooth, another phase of the sine pattern."""
    rng = np.random.default_rng(seed + 100)
    ws = rng.random(H * W).astype(np.float32)
    if kind == "flat":
        want = y.astype(np.float64) + 1e-3 * (rng.random((H, W, 3)) - 0.5)
    elif kind == "noise":
        want = rng.normal(0.3, 0.5, (H, W, 3))
    else:
        want = smooth(H, W, 0.4) + 0.02 * rng.random((H, W, 3))
    image = want.reshape(-1, 3).astype(np.float32) - ((np.float32(1) - ws) * np.float32(bg))[:, None]
    return torch.from_numpy(image.astype(np.float32)).contiguous(), torch.from_numpy(ws)


def blend_np(image, ws, bg, H, W):
    """x of the kernel: image + (1 - weights_sum) * bg in numpy float32 -> [H, W, 3]."""
    c = image.numpy() + ((np.float32(1) - ws.numpy()) * np.float32(bg))[:, None]
    assert c.dtype == np.float32
    return c.reshape(H, W, 3)


def direct_map(x, y):
    """The SSIM map with every windowed mean as one 121-tap double sum of the
    outer product of the 1-D weights (no separable passes)."""
    from nerf.eval import ssim_weights
    g = ssim_weights()
    w2 = np.outer(g, g)
    H, W = x.shape[:2]
    x, y = x.astype(np.float64), y.astype(np.float64)

    def window(a):
        out = np.zeros((H - HALO, W - HALO, 3))
        for i in range(11):
            for j in range(11):
                out += w2[i, j] * a[i:i + H - HALO, j:j + W - HALO]
        return out

    mux, muy = window(x), window(y)
    sx, sy, sxy = window(x * x) - mux * mux, window(y * y) - muy * muy, window(x * y) - mux * muy
    return ((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sx + sy + C2))
