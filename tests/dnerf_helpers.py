"""Restatements and fixtures for the D-NeRF tests (csrc/dnerf.hip, dnerf/):
the query points' arithmetic, the EMA / mean / pack over every slice and the
(x, t) encoding in numpy, the network's forward as a composition of the
repository's own operators, a torch restatement of one grid update, and a small
analytic dynamic scene (a sphere whose centre moves along x with time)."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import dnerf  # noqa: F401  (every D-NeRF test module imports the package)

X_OCTAVES, T_OCTAVES, ENCODE_COLS = 10, 6, 76


# ---- Morton codes --------------------------------------------------------------
def morton3(x, y, z):
    def expand(v):
        v = (v * 0x00010001) & 0xFF0000FF
        v = (v * 0x00000101) & 0x0F00F00F
        v = (v * 0x00000011) & 0xC30C30C3
        v = (v * 0x00000005) & 0x49249249
        return v
    x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
    return expand(x) | (expand(y) << 1) | (expand(z) << 2)


def morton3_invert(m):
    def compact(v):
        v = v & 0x09249249
        v = (v ^ (v >> 2)) & 0x030C30C3
        v = (v ^ (v >> 4)) & 0x0300F00F
        v = (v ^ (v >> 8)) & 0xFF0000FF
        v = (v ^ (v >> 16)) & 0x000003FF
        return v
    m = np.asarray(m, np.int64)
    return np.stack([compact(m), compact(m >> 1), compact(m >> 2)], -1)


# ---- query points ----------------------------------------------------------------
def cascade_scales(cas, H, bound):
    """(float32(bound_c - hgs), float32(hgs)) of a cascade, from Python floats as the renderer computes them."""
    bc = min(float(2 ** cas), float(bound))
    hgs = bc / H
    return np.float32(bc - hgs), np.float32(hgs)


def point_position(coords, u, cas, H, bound):
    """(2 c / (H - 1) - 1) (bound_c - hgs) + (2 u - 1) hgs with the kernel's fp32 operations.
    coords int [n, 3], u float32 [n, 3] in [0, 1)."""
    s, h = cascade_scales(cas, H, bound)
    inv = np.float32(1.0) / np.float32(H - 1)
    x = np.float32(2.0) * np.asarray(coords).astype(np.float32)
    x = x * inv
    x = x - np.float32(1.0)
    x = x * s
    j = np.asarray(u, np.float32) * np.float32(2.0)
    j = j - np.float32(1.0)
    j = j * h
    return (x + j).astype(np.float32)


def cell_centre64(coords, cas, H, bound):
    """The centre the jitter is added to, and hgs, in float64."""
    bc = min(float(2 ** cas), float(bound))
    hgs = bc / H
    return (2.0 * np.asarray(coords, np.float64) / (H - 1) - 1.0) * (bc - hgs), hgs


def point_time(t, T, u):
    """(t + 0.5) / T + (2 u - 1) 0.5 / T in fp32, kept inside [float32(t) / T, float32(t + 1) / T]."""
    fT = np.float32(T)
    centre = (np.asarray(t).astype(np.float32) + np.float32(0.5)) / fT
    hts = np.float32(0.5) / fT
    j = np.asarray(u, np.float32) * np.float32(2.0)
    j = (j - np.float32(1.0)) * hts
    tm = centre + j
    lo = np.asarray(t).astype(np.float32) / fT
    hi = (np.asarray(t) + 1).astype(np.float32) / fT
    return np.minimum(np.maximum(tm, lo), hi).astype(np.float32)


def slice_bounds32(t, T):
    """[t / T, (t + 1) / T] as float32 evaluates the two ends."""
    fT = np.float32(T)
    return np.asarray(t).astype(np.float32) / fT, (np.asarray(t) + 1).astype(np.float32) / fT


# ---- EMA, mean, pack ---------------------------------------------------------------
def ema_pack_ref(grid, tmp, decay, density_thresh):
    """grid, tmp float32 [T, C, H^3] -> (new grid, new tmp, float64 sum, float32 mean, bitfield uint8 [T, C H^3 / 8]).
    The threshold is Python's min(mean, density_thresh) over the WHOLE grid's mean."""
    grid = np.array(grid, np.float32)
    tmp = np.asarray(tmp, np.float32)
    valid = (grid >= 0) & (tmp >= 0)
    prod = grid * np.float32(decay)
    new = np.where(prod > tmp, prod, tmp)
    new = np.where(np.isnan(prod) | np.isnan(tmp), np.float32("nan"), new)
    grid = np.where(valid, new, grid).astype(np.float32)
    total = float(np.where(grid < 0, 0.0, grid.astype(np.float64)).sum(dtype=np.float64))
    mean = np.float32(total / grid.size)
    m, th = float(mean), float(density_thresh)
    thresh = np.float32(th if th < m else m)
    with np.errstate(invalid="ignore"):
        occ = (grid > thresh).reshape(grid.shape[0], -1, 8)
    bits = np.zeros(occ.shape[:2], np.uint8)
    for k in range(8):
        bits |= occ[:, :, k].astype(np.uint8) << k
    return grid, np.full_like(tmp, -1.0), total, mean, bits


# ---- encoding ------------------------------------------------------------------------
def encode_ref(x, t):
    """float64 [N, 76]: x, then per octave f < 10 sin(2^f x), cos(2^f x); then t with 6 octaves.
    x [N, 3], t [N] or [N, 1], float32 values taken to float64 exactly."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.float64).reshape(-1, 1)
    t = np.broadcast_to(t, (x.shape[0], 1)) if t.shape[0] == 1 else t
    cols = [x]
    for f in range(X_OCTAVES):
        cols += [np.sin(x * 2.0 ** f), np.cos(x * 2.0 ** f)]
    cols.append(t)
    for f in range(T_OCTAVES):
        cols += [np.sin(t * 2.0 ** f), np.cos(t * 2.0 ** f)]
    return np.concatenate(cols, 1)


def torch_encode(x, t):
    """The repository's plain-torch frequency encoders (encoding.FreqEncoder) on (x, t), in the inputs' dtype."""
    from encoding import FreqEncoder
    ex = FreqEncoder(3, X_OCTAVES - 1, X_OCTAVES)
    et = FreqEncoder(1, T_OCTAVES - 1, T_OCTAVES)
    assert ex.freq_bands == [2.0 ** f for f in range(X_OCTAVES)] and et.freq_bands == [2.0 ** f for f in range(T_OCTAVES)]
    t = t.reshape(-1, 1)
    if t.shape[0] == 1:
        t = t.expand(x.shape[0], 1)
    return torch.cat([ex(x), et(t)], 1)


def half_ulp(v):
    """The spacing of float16 at |v| (float64 array)."""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def encode_inputs(N, device, seed=0, bound=2.0):
    """x [N, 3] with 0 and +-bound in its first rows, the rest uniform in [-2, 2]^3; t [N, 1] with 0, 1, uniform."""
    g = torch.Generator().manual_seed(seed + N)
    x = torch.rand(N, 3, generator=g) * 4 - 2
    t = torch.rand(N, 1, generator=g)
    special = torch.tensor([[0.0, bound, -bound], [bound, -bound, 0.0], [-bound, 0.0, bound]])
    k = min(N, 3)
    x[:k] = special[:k]
    t[0] = 0.0
    if N > 1:
        t[1] = 1.0
    return x.to(device), t.to(device)


# ---- the network as a composition ----------------------------------------------------
def compose_forward(m, x, d, t):
    """NeRFNetwork.forward written out: the repository's (x, t) encoding, hash grid and SH encoders and F.linear
    on the model's weights (fp32, no autocast)."""
    from activation import trunc_exp

    def run(net, h):
        for l, layer in enumerate(net):
            h = F.linear(h, layer.weight)
            if l != len(net) - 1:
                h = F.relu(h)
        return h
    enc = dnerf.encode(x.contiguous(), t.contiguous())
    deform = run(m.deform_net, enc)
    g = m.encoder(x + deform, bound=m.bound)
    h = run(m.sigma_net, torch.cat([g, enc], 1))
    sigma, geo = trunc_exp(h[..., 0]), h[..., 1:]
    rgbs = torch.sigmoid(run(m.color_net, torch.cat([m.encoder_dir(d), geo], -1)))
    return sigma, rgbs, deform


@torch.no_grad()
def update_reference(m, decay=0.95):
    """One update_extra_state of the model's CURRENT state in plain torch, from the kernel's own points, times and
    indices (same chunks) -> (density_grid, mean_density) it must produce. The model is not changed."""
    T, C, H = m.time_size, m.cascade, m.grid_size
    grid = m.density_grid.clone()
    tmp = torch.full_like(grid, -1.0)
    partial, chunks = m.update_chunks()
    ws = dnerf.grid_points_workspace(T, C, H, grid.device) if partial else None
    for lo, hi in chunks:
        xyzs, times, indices = dnerf.grid_points(m.density_grid, T, C, H, m.bound, partial, m.grid_seed,
                                                 m.iter_density, lo, hi, ws)
        sigmas = m.density(xyzs, times.unsqueeze(-1))["sigma"].reshape(-1).float() * m.density_scale
        # a cell drawn more than once keeps its largest density (a float max; tmp starts at -1)
        tmp.view(-1).scatter_reduce_(0, indices.long(), sigmas, "amax", include_self=True)
    valid = (grid >= 0) & (tmp >= 0)
    grid[valid] = torch.maximum(grid[valid] * decay, tmp[valid])
    mean = np.float32(grid.clamp(min=0).double().sum().item() / grid.numel())
    return grid, float(mean)


# ---- a small dynamic scene ---------------------------------------------------------------
SCENE_R, SCENE_SCALE, SCENE_CAM = 0.25, 0.33, 4.0
SCENE_ANGLE_X = 0.6911112


def sphere_centre(time):
    """ngp coordinates: the centre moves along x with time in [0, 1]."""
    return np.array([-0.3 + 0.6 * float(time), 0.0, 0.0], np.float32)


def _blender_pose(k, n):
    th = 2 * math.pi * k / n
    ph = math.radians(25.0 + 10.0 * math.sin(3 * th))
    c = np.array([SCENE_CAM * math.cos(ph) * math.cos(th), SCENE_CAM * math.cos(ph) * math.sin(th),
                  SCENE_CAM * math.sin(ph)])
    back = c / np.linalg.norm(c)
    right = np.cross([0, 0, 1.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, back, c
    return c2w


def render_sphere(pose_ngp, intrinsics, H, W, time):
    """Analytic RGBA uint8 [H, W, 4] of the sphere at `time` from an ngp pose: the colour is the normal, alpha 1
    on the sphere and 0 elsewhere; the rays are the repository's get_rays'."""
    from nerf.utils import get_rays
    rays = get_rays(torch.from_numpy(pose_ngp[None]), intrinsics, H, W, -1)
    o = rays["rays_o"][0].double().numpy()
    d = rays["rays_d"][0].double().numpy()
    oc = o - sphere_centre(time).astype(np.float64)
    b = (oc * d).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - SCENE_R ** 2)
    hit = disc > 0
    tn = -b - np.sqrt(np.where(hit, disc, 0.0))
    hit &= tn > 0
    n = (oc + d * tn[:, None]) / SCENE_R
    rgba = np.zeros((H * W, 4))
    rgba[hit, :3] = 0.5 + 0.5 * n[hit]
    rgba[hit, 3] = 1.0
    return (rgba.reshape(H, W, 4) * 255).round().astype(np.uint8)


def write_scene(root, n_poses=8, n_times=4, res=32, test_frames=4, explicit_time=True):
    """A blender-format dynamic scene under `root`: transforms_train.json with n_poses x n_times frames and
    transforms_test.json with test_frames, RGBA PNGs, each frame's 'time' in [0, 1]."""
    from PIL import Image

    from nerf.provider import nerf_matrix_to_ngp
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    os.makedirs(os.path.join(root, "test"), exist_ok=True)
    focal = 0.5 * res / math.tan(0.5 * SCENE_ANGLE_X)
    intr = np.array([focal, focal, res / 2, res / 2], np.float32)

    def frames(split, items):
        out = []
        for i, (k, n, tm) in enumerate(items):
            c2w = _blender_pose(k, n)
            img = render_sphere(nerf_matrix_to_ngp(c2w.astype(np.float32), SCENE_SCALE), intr, res, res, tm)
            Image.fromarray(img, "RGBA").save(os.path.join(root, split, f"r_{i:03d}.png"))
            fr = {"file_path": f"./{split}/r_{i:03d}", "transform_matrix": c2w.tolist()}
            if explicit_time:
                fr["time"] = tm
            out.append(fr)
        return {"camera_angle_x": SCENE_ANGLE_X, "frames": out}

    times = [j / (n_times - 1) for j in range(n_times)]
    train = [(k, n_poses, tm) for tm in times for k in range(n_poses)]
    test = [(2 * j + 1, 2 * n_poses, (j + 0.5) / test_frames) for j in range(test_frames)]
    for split, items in (("train", train), ("test", test)):
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump(frames(split, items), f)
    return root


@torch.no_grad()
def scene_mse(model, dataset, fp16=True, max_steps=256):
    """Mean colour MSE over every frame of the dataset at its time: all its pixels marched as a training batch
    (no perturbation), blended on white."""
    from nerf.eval import ground_truth
    from nerf.utils import get_rays
    was = model.training
    model.train()
    n = int(dataset.poses.shape[0])
    acc = torch.zeros((), device=dataset.poses.device)
    for i in range(n):
        rays = get_rays(dataset.poses[i:i + 1], dataset.intrinsics, dataset.H, dataset.W, -1)
        with torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
            out = model.render(rays["rays_o"], rays["rays_d"], dataset.times[i:i + 1], bg_color=1, perturb=False,
                               force_all_rays=True, dt_gamma=0, max_steps=max_steps)
        acc += ((out["image"].float().reshape(-1, 3) - ground_truth(dataset, i)) ** 2).mean()
    total = float(acc.item()) / n
    model.train(was)
    return total
