"""Scenes with depth maps for the depth-supervision tests: SyntheticLego's
poses, its analytic target rendered on the CPU through get_rays and written as
PNGs with a transforms*.json (as tests/test_gpu_fused_images.py writes them),
plus one depth_k.npz per frame: the analytic distance along each pixel's
(unit) ray to the nearest box, 0 where the ray misses, in the units of the
file's poses."""
import json
import os

import numpy as np
import torch
from PIL import Image


def box_depth(lego, rays_o, rays_d):
    """Distance to the nearest box hit (SyntheticLego.target's slab test), 0 on a miss; [...]."""
    o = rays_o.reshape(-1, 1, 3)
    inv = 1.0 / rays_d.reshape(-1, 1, 3)
    t0 = (lego.box_lo[None] - o) * inv
    t1 = (lego.box_hi[None] - o) * inv
    tn = torch.minimum(t0, t1).amax(-1)
    tf = torch.maximum(t0, t1).amin(-1)
    tn = torch.where((tf >= tn) & (tf > 0), tn, torch.full_like(tn, float("inf")))
    tmin = tn.min(-1).values
    return torch.where(torch.isfinite(tmin), tmin, torch.zeros_like(tmin)).view(rays_o.shape[:-1])


def write_scene(path, n, H, W, channels=4, colmap=False, heldout=0, depth=True, no_depth=(), depth_dims=2,
                num_rays=1024):
    """n training views (+ `heldout` as the val split). depth: a dep_path per
    frame, except the frames in no_depth; depth_dims 3 stores [H, W, 1].
    colmap: one transforms.json with fx != fy and an off-centre principal point."""
    from nerf.provider import SyntheticLego
    from nerf.utils import get_rays
    lego = SyntheticLego(torch.device("cpu"), H=H, W=W, n_poses=n + heldout, num_rays=num_rays)
    intr = np.array([1.9 * W, 2.3 * H, 0.46 * W, 0.55 * H], np.float32) if colmap else lego.intrinsics
    frames = []
    for k in range(n + heldout):
        rays = get_rays(lego.poses[k:k + 1], intr, H, W, -1)
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
        fr = {"file_path": f"./r_{k}" + (".png" if colmap else ""), "transform_matrix": c2w.tolist()}
        if depth and k not in no_depth:
            d = box_depth(lego, rays["rays_o"], rays["rays_d"]).reshape(H, W).numpy().astype(np.float32)
            np.savez(os.path.join(path, f"depth_{k}.npz"), depth=d[..., None] if depth_dims == 3 else d)
            fr["dep_path"] = f"depth_{k}.npz"
        frames.append(fr)
    if colmap:
        t = {"fl_x": float(intr[0]), "fl_y": float(intr[1]), "cx": float(intr[2]), "cy": float(intr[3]), "h": H,
             "w": W, "frames": frames}
        with open(os.path.join(path, "transforms.json"), "w") as f:
            json.dump(t, f)
    else:
        for sp, fr in (("train", frames[:n]), ("val", frames[n:] or frames[:1])):
            with open(os.path.join(path, f"transforms_{sp}.json"), "w") as f:
                json.dump({"camera_angle_x": 0.6911112, "frames": fr}, f)
    return str(path)
