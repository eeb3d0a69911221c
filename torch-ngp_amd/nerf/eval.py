"""Evaluation of a trained model against a dataset's images: the reference's
eval_step (nerf/utils.py:636-642) on the device-driven test render."""
import math

import torch

from .fused_render import FusedRenderer
from .utils import get_rays


def ground_truth(dataset, index):
    """Image `index` as the reference's eval_step compares it: RGB as stored,
    RGBA blended on white (bg_color = 1), float32 [H * W, 3]."""
    img = dataset.images[index]
    img = img.float() / torch.full((1,), 255.0, device=img.device) if img.dtype == torch.uint8 else img.float()
    img = img.reshape(-1, img.shape[-1])
    if img.shape[-1] == 4:
        return img[:, :3] * img[:, 3:] + (1 - img[:, 3:])
    return img


@torch.no_grad()
def psnr(model, dataset, index, dt_gamma=0.0, renderer=None):
    """PSNR (-10 log10 of the MSE over every pixel and channel) of the model's
    render of pose `index` against the dataset's image: all H * W rays of the
    pose (get_rays), rendered on a white background. renderer: a FusedRenderer
    of H * W rays with its weights loaded, to reuse one across calls."""
    H, W = int(dataset.H), int(dataset.W)
    if renderer is None:
        renderer = FusedRenderer(model, H * W, dt_gamma=dt_gamma)
        renderer.load_weights()
    rays = get_rays(dataset.poses[index:index + 1], dataset.intrinsics, H, W, -1)
    out = renderer.render(rays["rays_o"], rays["rays_d"], bg_color=1)
    mse = float(((out["image"] - ground_truth(dataset, index)) ** 2).mean().item())
    return -10.0 * math.log10(mse) if mse > 0 else float("inf")
