"""Shared by the EMA / validation / schedule tests (test_gpu_ema.py,
test_gpu_validate.py, test_gpu_main_nerf_schedule.py): the scene writer of
tests/test_gpu_fused_images.py (SyntheticLego's poses, its analytic target
rendered on the CPU, quantised to uint8 PNGs with transforms_*.json), the
model and trainer those tests build, and a CPU restatement of torch_ema's
update."""
import json
import os

import numpy as np
import torch
from PIL import Image

N_RAYS = 1024
M_ROWS = 30000 + 128 - 30000 % 128  # 30000 rounded up to a multiple of 128


def write_scene(path, n, H, W, channels=4, heldout=0):
    """n training views (+ `heldout` more as the val split) of the Lego boxes."""
    from nerf.provider import SyntheticLego
    from nerf.utils import get_rays
    lego = SyntheticLego(torch.device("cpu"), H=H, W=W, n_poses=n + heldout, num_rays=N_RAYS)
    frames = []
    for k in range(n + heldout):
        rays = get_rays(lego.poses[k:k + 1], lego.intrinsics, H, W, -1)
        rgba = lego.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4)
        if channels == 3:  # RGB files show the solid on white
            rgba = rgba[..., :3] * rgba[..., 3:] + (1 - rgba[..., 3:])
        img = (rgba.numpy() * 255).round().astype(np.uint8)
        Image.fromarray(img, "RGBA" if channels == 4 else "RGB").save(os.path.join(path, f"r_{k}.png"))
        # the file's pose: the one nerf_matrix_to_ngp(scale=1) maps to SyntheticLego's
        P = lego.poses[k].numpy()
        c2w = np.eye(4)
        c2w[0], c2w[1], c2w[2] = P[2], P[0], P[1]
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": f"./r_{k}", "transform_matrix": c2w.tolist()})
    for sp, fr in (("train", frames[:n]), ("val", frames[n:] or frames[:1])):
        with open(os.path.join(path, f"transforms_{sp}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112, "frames": fr}, f)
    return str(path)


def dataset(path, dev, store="uint8", type="train"):
    from nerf.provider import NeRFDataset
    return NeRFDataset(path, dev, type=type, scale=1.0, num_rays=N_RAYS, store=store)


def model(dev):
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import lego_bitfield
    torch.manual_seed(0)
    m = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    with torch.no_grad():  # a non-trivial field: larger table values than the 1e-4 init
        m.encoder.embeddings.normal_(0, 0.05)
    m.density_bitfield.copy_(torch.from_numpy(lego_bitfield()).to(dev))
    return m


def trainer(dev, data, seed=3, **kw):
    from nerf.fused import FusedTrainer
    return FusedTrainer(model(dev), data, M=M_ROWS, seed=seed, **kw)


def bits(t):
    return t.contiguous().view(torch.int32)


def torch_ema_update(shadow, param, one_minus_decay):
    """torch_ema's ExponentialMovingAverage.update() on one CPU float32 tensor,
    operation for operation (in place on `shadow`)."""
    assert shadow.device.type == "cpu" and shadow.dtype == torch.float32 == param.dtype
    tmp = shadow - param
    tmp.mul_(float(one_minus_decay))
    shadow.sub_(tmp)
    return shadow


def torch_ema_decay(ema_decay, num_updates):
    """torch_ema's warm-up: the decay of update number `num_updates` (1-based)."""
    return min(ema_decay, (1 + num_updates) / (10 + num_updates))
