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
DEFAULT_S = S


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


def grid_levels(offsets=None, base=None, S=None):
    """Per level (scale, res, off0, hs, dense) of gridencoder's make_levels: scale
    = exp2f(level * S) * base - 1 in float32, res = ceil(scale) + 1; dense where
    (res + 1)^2 entries fit in the level's hs."""
    offsets = OFFSETS if offsets is None else [int(v) for v in offsets]
    base = BASE if base is None else base
    S = DEFAULT_S if S is None else S
    out = []
    for lv in range(LEVELS):
        scale = np.float32(np.float32(np.exp2(np.float64(np.float32(lv) * np.float32(S)))) * np.float32(base)
                           - np.float32(1))
        res = int(np.ceil(scale)) + 1
        off0, hs = offsets[lv], offsets[lv + 1] - offsets[lv]
        out.append((scale, res, off0, hs, (res + 1) ** 2 <= hs))
    return out


def grid_corners64(x01, offsets=None, base=None, S=None):
    """The 2-D hash grid's indexing (4 levels, bilinear, align_corners off, hash
    where the dense level would not fit) at x01 [N, 2] in [0, 1]: per level
    (entries [N, 4] int64, rows of the whole table, weights [N, 4] float64)."""
    x01 = np.asarray(x01, dtype=np.float64)
    out = []
    for scale, res, off0, hs, dense in grid_levels(offsets, base, S):
        pos = x01 * np.float64(scale) + 0.5
        pg = np.floor(pos).astype(np.int64)
        fr = pos - pg
        e = np.zeros((x01.shape[0], 4), dtype=np.int64)
        w = np.ones((x01.shape[0], 4))
        for idx in range(4):
            pl = np.zeros_like(pg)
            for dd in range(2):
                if idx & (1 << dd):
                    w[:, idx] *= fr[:, dd]
                    pl[:, dd] = pg[:, dd] + 1
                else:
                    w[:, idx] *= 1 - fr[:, dd]
                    pl[:, dd] = pg[:, dd]
            if dense:  # stride res + 1
                index = pl[:, 0] + pl[:, 1] * (res + 1)
            else:  # fast_hash, primes 1 and 2654435761, in uint32
                index = ((pl[:, 0] & 0xffffffff) ^ ((pl[:, 1] * 2654435761) & 0xffffffff)) & 0xffffffff
            e[:, idx] = off0 + index % hs
        out.append((e, w))
    return out


def grid64(x01, table, offsets=None, base=None, S=None):
    """Float64 interpolation of `table` [entries, 2] at x01 [N, 2] in [0, 1],
    through grid_corners64 -> [N, 8]."""
    out = np.zeros((x01.shape[0], 2 * LEVELS))
    for lv, (e, w) in enumerate(grid_corners64(x01, offsets, base, S)):
        for idx in range(4):
            out[:, 2 * lv:2 * lv + 2] += w[:, idx, None] * table[e[:, idx]]
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


def features64(o, d, radius, table_half, offsets=None, base=None, S=None):
    """The MLP's input row in float64: [SH4(d) | grid(sph01) | 0 (8)] -> [N, 32]."""
    x01 = (sph64(o, d, radius) + 1) / 2
    grid = grid64(x01, table_half.astype(np.float64), offsets, base, S)
    return np.concatenate([sh4(d), grid, np.zeros((o.shape[0], 8))], 1)


def split_weights(weights_half):
    """The flat weights -> W0 [64, 32], W1 [16, 64] in float64."""
    w = np.asarray(weights_half).astype(np.float64)
    return w[:64 * 32].reshape(64, 32), w[64 * 32:].reshape(16, 64)


def mlp64(feat, weights_half):
    """sigmoid(W1[:3] relu(W0 x)) in float64 -> [N, 3]."""
    w0, w1 = split_weights(weights_half)
    h = np.maximum(feat @ w0.T, 0)
    return 1 / (1 + np.exp(-(h @ w1.T)[:, :3]))


def background64(o, d, radius, table_half, weights_half, offsets=None, base=None, S=None):
    """The model in float64 on the fp16-rounded table and weights (float64
    copies of the half values): what every fp16 path approximates. -> [N, 3]."""
    return mlp64(features64(o, d, radius, table_half, offsets, base, S), weights_half)


def uncertain_units(x, weights_half):
    """[N, 64] bool: hidden units whose float64 pre-activation h = W0 x lies
    within 64 * 2^-24 * sum |w| |x| of zero, twice the worst-case error of a
    32-term fp32 dot product: an fp32 evaluation could put the ReLU's mask the
    other way there."""
    w0, _ = split_weights(weights_half)
    x = np.asarray(x).astype(np.float64)
    return np.abs(x @ w0.T) < 64 * 2.0 ** -24 * (np.abs(x) @ np.abs(w0).T)


def bwd_blocks(N):
    """Workgroups of the backward launch: 256 rays each, at most 64."""
    return min((N + 255) // 256, 64)


def background_backward64(x_half, sph01, bg, out_image, out_ws, gt, weights_half, scale, color_weight, N, offsets=None,
                          base=None, S=None, order=None, faithful=False):
    """d (scale * cw * mean((out_image - gt[:, :3])^2)) / d (table, W0, W1[:3]) of
    the background model in float64, from what the backward reads: the saved
    input rows x [N, 32], sph01 [N, 2], bg [N, 3], the composite's out_image
    [N, 3] and out_ws [N], gt [N, 4], the weights:
        G = scale cw / N / 3,  gy = G 2 (out_image - gt) (1 - out_ws) bg (1 - bg),
        h = W0 x,  delta = [h > 0] W1[:3]^T gy,  dW1 = gy^T relu(h),  dW0 = delta^T x,
        gi = W0[:, 16:24]^T delta,  table[e] += w_corner gi[2 l : 2 l + 2]
    (rays whose sph01 leaves [0, 1] scatter nothing). `order` is the ray-index
    column of a rays list: one term per entry inside [0, N), none for the rest;
    None is the identity. -> (g_table [entries, 2], g_w0 [64, 32], g_w1 [3, 64]).

    faithful: gy, relu(h), delta and gi are rounded to fp16 where the kernel
    rounds them, everything else stays float64; a fourth value is returned, the
    dict of each output's bound terms: S_* the same expression with every
    factor's absolute value from gy on, n_table the scatter terms per entry
    and n_w the workgroups that add to each dW value."""
    offsets = OFFSETS if offsets is None else [int(v) for v in offsets]
    idx = np.arange(N) if order is None else np.asarray(order).astype(np.int64).reshape(-1)
    idx = idx[(idx >= 0) & (idx < N)]
    f64 = lambda a: np.asarray(a).astype(np.float64)  # noqa: E731
    r16 = (lambda a: a.astype(np.float16).astype(np.float64)) if faithful else (lambda a: a)
    x, y, ws = f64(x_half)[idx], f64(bg)[idx], f64(out_ws)[idx]
    w0, w1 = split_weights(weights_half)
    w1, w0g = w1[:3], w0[:, 16:24]
    G = float(scale) * float(color_weight) / N / 3
    gy = r16(G * 2 * (f64(out_image)[idx] - f64(gt)[idx, :3]) * (1 - ws)[:, None] * (y * (1 - y)))
    h = x @ w0.T
    live = h > 0
    act = r16(np.maximum(h, 0))
    delta = r16(live * (gy @ w1))
    gi = r16(delta @ w0g)
    a_delta = live * (np.abs(gy) @ np.abs(w1))
    a_gi = a_delta @ np.abs(w0g)
    g_table, s_table = np.zeros((offsets[-1], 2)), np.zeros((offsets[-1], 2))
    n_table = np.zeros(offsets[-1], dtype=np.int64)
    sp = f64(sph01)[idx]
    inside = ((sp >= 0) & (sp <= 1)).all(1)
    for lv, (e, w) in enumerate(grid_corners64(sp[inside], offsets, base, S)):
        for k in range(4):
            for c in range(2):
                np.add.at(g_table[:, c], e[:, k], w[:, k] * gi[inside, 2 * lv + c])
                np.add.at(s_table[:, c], e[:, k], np.abs(w[:, k]) * a_gi[inside, 2 * lv + c])
            np.add.at(n_table, e[:, k], 1)
    out = (g_table, delta.T @ x, gy.T @ act)
    if not faithful:
        return out
    return out + (dict(S_table=s_table, S_w0=a_delta.T @ np.abs(x), S_w1=np.abs(gy).T @ act, n_table=n_table,
                       n_w=bwd_blocks(N)),)


def fp16_spacing(a):
    """The distance between neighbouring fp16 numbers at |a| (2^-24 below 2^-14)."""
    return np.exp2(np.maximum(np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -30))), -14.0) - 10)


def backward_tolerance(ref, S, n):
    """4 * 2^-11 * S (three chained fp16 roundings that may fall the other way
    and the fp32 accumulation) + n * 2^-25 (half a unit of the 2^-24 fixed
    point per atomic contribution) + the fp16 spacing at |ref| (the final store)."""
    return 4 * 2.0 ** -11 * S + np.asarray(n, dtype=np.float64) * 2.0 ** -25 + fp16_spacing(ref)


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
