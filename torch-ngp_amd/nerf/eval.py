"""Evaluation of a trained model against a dataset's images: the reference's
eval_step (nerf/utils.py:636-642) on the device-driven test render; and
against its depth maps: the supervised depth term over a whole view."""
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


@torch.no_grad()
def depth_error(model, dataset, index, dt_gamma=0.0, max_steps=1024, chunk=4096):
    """Masked mean |gt - depth_bound_scale| over all H * W rays of pose `index`:
    the quantity depth supervision trains (nerf/utils.py:545-553), so it is
    computed with the training composite through the reference-API render
    (perturb=False, force_all_rays=True), the target dataset.depths[index] *
    depth_scale, the mask min_near <= gt <= bound. nan when no pixel of the
    view lies in the mask."""
    H, W = int(dataset.H), int(dataset.W)
    if getattr(dataset, "depths", None) is None:
        raise ValueError("depth_error: the dataset has no depth maps (dataset.depths)")
    rays = get_rays(dataset.poses[index:index + 1], dataset.intrinsics, H, W, -1)
    was_training = model.training
    model.train()  # the training composite (march_rays_train + composite_rays_train)
    local_step, counts = model.local_step, model.step_counter.clone()
    pred = []
    try:
        # force_all_rays sizes the sample buffers for max_steps samples per ray: a few thousand rays at a time
        for a in range(0, H * W, chunk):
            with torch.autocast("cuda", dtype=torch.float16):
                out = model.render(rays["rays_o"][:, a:a + chunk], rays["rays_d"][:, a:a + chunk], staged=False,
                                   bg_color=1, perturb=False, force_all_rays=True, dt_gamma=dt_gamma,
                                   max_steps=max_steps)
            pred.append(out["depth_bound_scale"].float())
    finally:
        # (run_cuda counted training steps: the trainer's bookkeeping stays as it was)
        model.local_step = local_step
        model.step_counter.copy_(counts)
        model.train(was_training)
    gt = dataset.depths[index].reshape(1, -1) * dataset.depth_scale
    mask = (model.min_near <= gt) & (gt <= model.bound)
    err = torch.abs(gt - torch.cat(pred, 1))[mask]
    return float(err.mean().item()) if err.numel() else float("nan")
