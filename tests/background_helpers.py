"""Helpers of the background-model tests: a float64 restatement of the model
(sph_from_ray, the 2-D hash grid, SH degree 4, the 32 -> 64 -> 3 MLP, the
sigmoid), written apart from the product code on purpose, and scenes whose
images show the Lego boxes over a smooth backdrop."""
import json
import os

import numpy as np
import torch
from PIL import Image

OFFSETS = [0, 296, 7024, 173488, 697776]
BASE, LEVELS = 16, 4
S = float(np.log2(np.exp2(np.log2(2048 / 16) / 3)))  # log2(per_level_scale) of GridEncoder(desired_resolution=2048)


def sph64(o, d, radius):
    """raymarching.sph_from_ray in float64 -> [N, 2] in [-1, 1]."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    A = (d * d).sum(1)
    B = (o * d).sum(1)
    C = (o * o).sum(1) - radius * radius
    t = (-B + np.sqrt(B * B - A * C)) / A
    p = o + t[:, None] * d
    theta = np.arctan2(np.sqrt(p[:, 0] ** 2 + p[:, 2] ** 2), p[:, 1])
    phi = np.arctan2(p[:, 2], p[:, 0])
    return np.stack([2 * theta / np.pi - 1, phi / np.pi], 1)


def grid64(x01, table):
    """The 2-D hash grid (4 levels x 2 features, bilinear, align_corners off,
    hash where the dense level would not fit) at x01 [N, 2] in [0, 1], float64
    interpolation of `table` [entries, 2] -> [N, 8]."""
    out = np.zeros((x01.shape[0], 2 * LEVELS))
    for lv in range(LEVELS):
        scale = np.float32(np.float32(np.exp2(np.float64(np.float32(lv) * np.float32(S)))) * np.float32(BASE)
                           - np.float32(1))
        res = int(np.ceil(scale)) + 1
        off0, hs = OFFSETS[lv], OFFSETS[lv + 1] - OFFSETS[lv]
        pos = x01 * np.float64(scale) + 0.5
        pg = np.floor(pos).astype(np.int64)
        fr = pos - pg
        for idx in range(4):
            w = np.ones(x01.shape[0])
            pl = np.zeros_like(pg)
            for dd in range(2):
                if idx & (1 << dd):
                    w = w * fr[:, dd]
                    pl[:, dd] = pg[:, dd] + 1
                else:
                    w = w * (1 - fr[:, dd])
                    pl[:, dd] = pg[:, dd]
            if (res + 1) ** 2 <= hs:  # dense: stride res + 1
                index = pl[:, 0] + pl[:, 1] * (res + 1)
            else:  # fast_hash, primes 1 and 2654435761, in uint32
                index = ((pl[:, 0] & 0xffffffff) ^ ((pl[:, 1] * 2654435761) & 0xffffffff)) & 0xffffffff
            e = off0 + index % hs
            out[:, 2 * lv:2 * lv + 2] += w[:, None] * table[e]
    return out


def sh4(d):
    """The 16 real SH basis functions of degree < 4 at d [N, 3] (float64)."""
    x, y, z = d[:, 0].astype(np.float64), d[:, 1].astype(np.float64), d[:, 2].astype(np.float64)
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return np.stack([
        np.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z,
        -0.48860251190291987 * x, 1.0925484305920792 * xy, -1.0925484305920792 * yz,
        0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
        0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2),
        2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1.0 - 5.0 * z2),
        0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)], 1)


def background64(o, d, radius, table_half, weights_half):
    """The model in float64 on the fp16-rounded table and weights (float64
    copies of the half values): what every fp16 path approximates. -> [N, 3]."""
    x01 = (sph64(o, d, radius) + 1) / 2
    feat = np.concatenate([sh4(d), grid64(x01, table_half.astype(np.float64)), np.zeros((o.shape[0], 8))], 1)
    w = weights_half.astype(np.float64)
    w0, w1 = w[:64 * 32].reshape(64, 32), w[64 * 32:].reshape(16, 64)
    h = np.maximum(feat @ w0.T, 0)
    return 1 / (1 + np.exp(-(h @ w1.T)[:, :3]))


def backdrop(d):
    """A smooth colour per (unit) ray direction, in [0.1, 0.9]: torch [.., 3]."""
    d = d / d.norm(dim=-1, keepdim=True)
    return 0.5 + 0.4 * torch.stack([torch.sin(2.0 * d[..., 0] + 0.3), torch.cos(1.5 * d[..., 1] - 0.2),
                                    torch.sin(1.7 * d[..., 2] + 1.0)], -1)


def write_backdrop_scene(path, n, H, W, heldout=1, num_rays=1024):
    """n training views and `heldout` val views of the Lego boxes composited
    over backdrop(ray direction), from the dataset's own rays, as RGB PNGs with
    transforms_{train,val}.json (depth_helpers.write_scene's pose convention)."""
    from nerf.provider import SyntheticLego
    from nerf.utils import get_rays
    lego = SyntheticLego(torch.device("cpu"), H=H, W=W, n_poses=n + heldout, num_rays=num_rays)
    frames = []
    for k in range(n + heldout):
        rays = get_rays(lego.poses[k:k + 1], lego.intrinsics, H, W, -1)
        rgba = lego.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4)
        sky = backdrop(rays["rays_d"].reshape(H, W, 3))
        rgb = rgba[..., :3] * rgba[..., 3:] + sky * (1 - rgba[..., 3:])
        Image.fromarray((rgb.numpy() * 255).round().astype(np.uint8), "RGB").save(os.path.join(path, f"r_{k}.png"))
        P = lego.poses[k].numpy()
        c2w = np.eye(4)
        c2w[0], c2w[1], c2w[2] = P[2], P[0], P[1]
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": f"./r_{k}", "transform_matrix": c2w.tolist()})
    for sp, fr in (("train", frames[:n]), ("val", frames[n:])):
        with open(os.path.join(path, f"transforms_{sp}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112, "frames": fr}, f)
    return str(path)
