"""Synthetic 'Lego-like' dataset (SURVEY §8(d) Config 2): the real
nerf_synthetic/lego images are not available offline, so the scene is an
analytic solid (union of three coloured boxes) seen from 100 ring poses in
the nerf_synthetic convention, converted with nerf_matrix_to_ngp exactly as
the reference provider does (nerf/provider.py:19-27). Rays/targets are
produced on the GPU each step like the reference's preload + collate path
(provider.py:442-564, utils.py:52-136)."""
import math

import numpy as np
import torch

from .utils import get_rays

LEGO_BOXES = [((-0.5, -0.35, -0.3), (0.5, 0.35, 0.1)),
              ((-0.2, -0.2, 0.1), (0.2, 0.2, 0.45)),
              ((-0.45, -0.3, -0.3), (-0.25, 0.3, 0.3))]
LEGO_COLORS = [(0.95, 0.75, 0.1), (0.8, 0.1, 0.1), (0.3, 0.3, 0.3)]


def nerf_matrix_to_ngp(pose, scale=0.33, offset=(0, 0, 0)):
    return np.array([
        [pose[1, 0], -pose[1, 1], -pose[1, 2], pose[1, 3] * scale + offset[0]],
        [pose[2, 0], -pose[2, 1], -pose[2, 2], pose[2, 3] * scale + offset[1]],
        [pose[0, 0], -pose[0, 1], -pose[0, 2], pose[0, 3] * scale + offset[2]],
        [0, 0, 0, 1]], dtype=np.float32)


def _quat_from_matrix(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix, float64: the branch
    with the largest divisor (Shepperd), so no case loses digits."""
    R = np.asarray(R, dtype=np.float64)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    k = int(np.argmax([t, R[0, 0], R[1, 1], R[2, 2]]))
    if k == 0:
        q = np.array([1 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1 + 2 * R[0, 0] - t, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1 + 2 * R[1, 1] - t, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 + 2 * R[2, 2] - t])
    return q / np.linalg.norm(q)


def _matrix_from_quat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def interpolate_poses(pose0, pose1, n):
    """A camera path between two poses for scenes without a test split, the
    reference's rule (nerf/provider.py:208-222): for i = 0..n the ratio
    sin((i / n - 0.5) * pi) * 0.5 + 0.5 (slow at both ends), the rotation
    slerped along the shorter arc (scipy's Slerp there, quaternions here), the
    translation interpolated linearly. -> float32 [n + 1, 4, 4]."""
    n = int(n)
    if n < 1:
        raise ValueError(f"interpolate_poses: n must be >= 1, got {n}")
    pose0, pose1 = np.asarray(pose0, dtype=np.float64), np.asarray(pose1, dtype=np.float64)
    q0, q1 = _quat_from_matrix(pose0[:3, :3]), _quat_from_matrix(pose1[:3, :3])
    dot = float(np.dot(q0, q1))
    if dot < 0:  # q and -q are one rotation: take the shorter arc
        q1, dot = -q1, -dot
    theta = math.acos(min(dot, 1.0))  # half the angle between the rotations
    out = np.zeros((n + 1, 4, 4), dtype=np.float32)
    for i in range(n + 1):
        ratio = math.sin((i / n - 0.5) * math.pi) * 0.5 + 0.5
        if theta < 1e-6:  # sin(theta) ~ 0: the chord is the arc
            q = (1 - ratio) * q0 + ratio * q1
        else:
            q = (math.sin((1 - ratio) * theta) * q0 + math.sin(ratio * theta) * q1) / math.sin(theta)
        out[i, :3, :3] = _matrix_from_quat(q / np.linalg.norm(q))
        out[i, :3, 3] = (1 - ratio) * pose0[:3, 3] + ratio * pose1[:3, 3]
        out[i, 3, 3] = 1
    return out


def _morton3(x, y, z):
    def expand(v):
        v = (v * 0x00010001) & 0xFF0000FF
        v = (v * 0x00000101) & 0x0F00F00F
        v = (v * 0x00000011) & 0xC30C30C3
        v = (v * 0x00000005) & 0x49249249
        return v
    x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
    return expand(x) | (expand(y) << 1) | (expand(z) << 2)


def box_bitfield(boxes=LEGO_BOXES, cascade=1, H=128, bound=1.0):
    """Occupancy bitfield [C*H^3/8] (Morton order, like packbits): a cell is
    occupied when its centre lies in any box; cascade c spans min(2^c, bound)."""
    i = np.arange(H)
    xx, yy, zz = (a.reshape(-1) for a in np.meshgrid(i, i, i, indexing="ij"))
    idx = _morton3(xx, yy, zz)
    grid = np.zeros((cascade, H ** 3), np.float32)
    for c in range(cascade):
        b = min(2 ** c, bound)
        cx, cy, cz = (((a + 0.5) / H * 2 - 1) * b for a in (xx, yy, zz))
        occ = np.zeros(H ** 3, bool)
        for lo, hi in boxes:
            occ |= ((cx >= lo[0]) & (cx <= hi[0]) & (cy >= lo[1]) & (cy <= hi[1]) &
                    (cz >= lo[2]) & (cz <= hi[2]))
        grid[c, idx] = occ
    flat = grid.reshape(-1, 8)
    bits = np.zeros(flat.shape[0], np.uint8)
    for k in range(8):
        bits |= (flat[:, k] > 0.5).astype(np.uint8) << k
    return bits


def lego_bitfield(cascade=1, H=128, bound=1.0):
    return box_bitfield(LEGO_BOXES, cascade, H, bound)


def sphere_bitfield(radius=0.7, cascade=1, H=128, bound=1.0):
    """Occupancy of the cells whose centre lies in a ball (a conservative,
    early-training grid around the Lego boxes, which it contains): ~80 samples
    per ray at the Lego cameras, inside SURVEY §8(d)'s 50-120 estimate."""
    i = np.arange(H)
    xx, yy, zz = (a.reshape(-1) for a in np.meshgrid(i, i, i, indexing="ij"))
    idx = _morton3(xx, yy, zz)
    grid = np.zeros((cascade, H ** 3), np.float32)
    for c in range(cascade):
        b = min(2 ** c, bound)
        cx, cy, cz = (((a + 0.5) / H * 2 - 1) * b for a in (xx, yy, zz))
        grid[c, idx] = (cx * cx + cy * cy + cz * cz) <= radius * radius
    flat = grid.reshape(-1, 8)
    bits = np.zeros(flat.shape[0], np.uint8)
    for k in range(8):
        bits |= (flat[:, k] > 0.5).astype(np.uint8) << k
    return bits


# A Fox-shaped solid for Config 3 (bound 2): head, snout, ears and body as
# ellipsoids (centre, radii) in ngp coordinates. The real data/fox images are
# not in the image; this occupancy gives the bench's Config-3 leg ~30 samples
# per ray at dt_gamma 1/128 from the ring cameras (62 % of rays hit it), where
# the Lego boxes at bound 2 give 2.7.
FOX_ELLIPSOIDS = [((0.0, 0.0, 0.13), (0.975, 0.78, 0.715)),
                  ((0.91, 0.0, -0.065), (0.585, 0.325, 0.286)),
                  ((-0.26, 0.455, 0.845), (0.195, 0.156, 0.39)),
                  ((-0.26, -0.455, 0.845), (0.195, 0.156, 0.39)),
                  ((-0.65, 0.0, -0.78), (0.91, 0.65, 0.65))]


def ellipsoid_bitfield(ellipsoids=FOX_ELLIPSOIDS, cascade=2, H=128, bound=2.0):
    """Occupancy of the cells whose centre lies in any ellipsoid (as
    box_bitfield: Morton order, cascade c spans min(2^c, bound))."""
    i = np.arange(H)
    xx, yy, zz = (a.reshape(-1) for a in np.meshgrid(i, i, i, indexing="ij"))
    idx = _morton3(xx, yy, zz)
    grid = np.zeros((cascade, H ** 3), np.float32)
    for c in range(cascade):
        b = min(2 ** c, bound)
        cx, cy, cz = (((a + 0.5) / H * 2 - 1) * b for a in (xx, yy, zz))
        occ = np.zeros(H ** 3, bool)
        for (x0, y0, z0), (rx, ry, rz) in ellipsoids:
            occ |= ((cx - x0) / rx) ** 2 + ((cy - y0) / ry) ** 2 + ((cz - z0) / rz) ** 2 <= 1
        grid[c, idx] = occ
    flat = grid.reshape(-1, 8)
    bits = np.zeros(flat.shape[0], np.uint8)
    for k in range(8):
        bits |= (flat[:, k] > 0.5).astype(np.uint8) << k
    return bits


def fox_bitfield(cascade=2, H=128, bound=2.0):
    return ellipsoid_bitfield(FOX_ELLIPSOIDS, cascade, H, bound)


class SyntheticLego:
    """100 ring poses at 800x800, camera_angle_x 0.6911112, radius 4.0311
    (scaled by `scale`, default 0.8 as in readme.md:139)."""

    def __init__(self, device, H=800, W=800, n_poses=100, scale=0.8, radius=4.0311,
                 camera_angle_x=0.6911112, num_rays=4096):
        self.device = device
        self.H, self.W = H, W
        self.num_rays = num_rays
        focal = 0.5 * W / math.tan(0.5 * camera_angle_x)
        self.intrinsics = np.array([focal, focal, W / 2, H / 2], dtype=np.float32)
        poses = []
        for k in range(n_poses):
            th = 2 * math.pi * k / n_poses
            ph = math.radians(30.0 + 15.0 * math.sin(3 * th))
            c = np.array([radius * math.cos(ph) * math.cos(th), radius * math.cos(ph) * math.sin(th),
                          radius * math.sin(ph)])
            back = c / np.linalg.norm(c)
            right = np.cross([0, 0, 1.0], back); right /= np.linalg.norm(right)
            up = np.cross(back, right)
            c2w = np.eye(4)
            c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, back, c
            poses.append(nerf_matrix_to_ngp(c2w, scale=scale))
        self.poses = torch.from_numpy(np.stack(poses)).to(device)
        lo = torch.tensor([b[0] for b in LEGO_BOXES], device=device)
        hi = torch.tensor([b[1] for b in LEGO_BOXES], device=device)
        # the solid lives in ngp coordinates already (x, y, z of the bound box)
        self.box_lo, self.box_hi = lo, hi
        self.box_rgb = torch.tensor(LEGO_COLORS, device=device)

    def target(self, rays_o, rays_d):
        """Analytic RGBA: colour of the nearest box hit, alpha 1; else alpha 0."""
        o = rays_o.reshape(-1, 1, 3)
        inv = 1.0 / rays_d.reshape(-1, 1, 3)
        t0 = (self.box_lo[None] - o) * inv
        t1 = (self.box_hi[None] - o) * inv
        tn = torch.minimum(t0, t1).amax(-1)
        tf = torch.maximum(t0, t1).amin(-1)
        hit = (tf >= tn) & (tf > 0)
        tn = torch.where(hit, tn, torch.full_like(tn, float("inf")))
        tmin, arg = tn.min(-1)
        alpha = torch.isfinite(tmin).float()
        rgb = self.box_rgb[arg] * alpha[:, None]
        return torch.cat([rgb, alpha[:, None]], -1).view(*rays_o.shape[:-1], 4)

    def sample(self, index=None):
        """One training batch: rays of `num_rays` random pixels of one random
        pose. Device-side RNG only (no host sync), so it can sit in a graph."""
        if index is None:
            index = torch.randint(0, self.poses.shape[0], (1,), device=self.device)
        else:
            index = torch.tensor([index], device=self.device)
        poses = self.poses.index_select(0, index)
        rays = get_rays(poses, self.intrinsics, self.H, self.W, self.num_rays)
        images = self.target(rays["rays_o"], rays["rays_d"])
        return {"H": self.H, "W": self.W, "rays_o": rays["rays_o"], "rays_d": rays["rays_d"],
                "images": images}


class NeRFDataset:
    """Real-scene loader for the reference's transforms*.json format
    (nerf/provider.py:127-440): blender splits (transforms_{train,val,test}.json,
    'trainval' = train + val) or one colmap-style transforms.json. Poses go
    through nerf_matrix_to_ngp(scale, offset) (:19-27); images are decoded with
    PIL (the reference uses cv2, absent here) to float RGB(A) / 255 and
    area-resized by 1/downscale (cv2.INTER_AREA there, PIL's box filter here);
    intrinsics come from fl_x/fl_y or camera_angle_x/y, cx/cy defaulting to the
    image centre (:419-434). sample() is the reference's collate for training
    (:442-508): num_rays random pixels of one random image, through get_rays,
    with their ground-truth colours gathered; on the GPU the same batch feeds
    nerf.train.Trainer exactly like SyntheticLego does.
    store: how `images` [n, H, W, C] is kept on the device: "float32" (v / 255)
    or "uint8" (the decoded bytes, a quarter of the memory; sample() and the
    fused engine's image source divide by 255 as they gather, the same values
    bit for bit).
    Depth maps (the reference's dep_path, :346-357, 390-391): a frame's
    `dep_path` names an .npz whose `depth` is [H, W] or [H, W, 1]; the maps are
    stacked into `depths` [n, H, W] float32 on the device, in file units,
    nearest-resized with the images (cv2.INTER_NEAREST's rule: source index
    floor(i * src / dst)). Every frame has one or none has (`depths` None).
    depth_scale: file units -> ngp units, gt = depth * depth_scale (default: the
    pose `scale`; the reference's 2 * bound / aabb_size is the caller's to
    pass); sample() returns "depths" [1, N] in ngp units (:555-557).
    error_map (the reference's --error_map, :397-401): for type "train",
    `error_map` is a float32 [n, error_map_res ** 2] tensor of ones on the
    device, a coarse error image per view, cell = row_cell * res + col_cell;
    otherwise None. sample() then draws its pixels from the map (get_rays'
    error_map branch) and returns their cells as "inds_coarse"; the trainers
    fold each ray's loss back into the map. error_map_res: 1..128 (the
    reference's fixed 128)."""

    def __init__(self, path, device, type="train", downscale=1, scale=0.33, offset=(0, 0, 0), num_rays=4096,
                 store="float32", depth_scale=None, error_map=False, error_map_res=128):
        import json
        import os

        from PIL import Image

        if store not in ("float32", "uint8"):
            raise ValueError(f"NeRFDataset: store must be 'float32' or 'uint8', got {store!r}")
        self.device, self.num_rays, self.store = device, num_rays, store
        self.error_map_res = int(error_map_res)
        if error_map_res != self.error_map_res or not 1 <= self.error_map_res <= 128:
            raise ValueError(f"NeRFDataset: error_map_res must be an integer in 1..128, got {error_map_res!r}")
        if os.path.exists(os.path.join(path, "transforms.json")):
            self.mode = "colmap"
            with open(os.path.join(path, "transforms.json")) as f:
                transform = json.load(f)
            frames = transform["frames"]
        elif os.path.exists(os.path.join(path, "transforms_train.json")):
            self.mode = "blender"
            splits = ["train", "val"] if type == "trainval" else [type]
            frames, transform = [], None
            for sp in splits:
                with open(os.path.join(path, f"transforms_{sp}.json")) as f:
                    t = json.load(f)
                transform = transform or t
                frames += t["frames"]
        else:
            raise FileNotFoundError(f"NeRFDataset: no transforms*.json under {path}")
        H = W = None
        if "h" in transform and "w" in transform:
            H, W = int(transform["h"]) // downscale, int(transform["w"]) // downscale
        poses, images, depths, no_depth = [], [], [], None
        for fr in frames:
            fp = os.path.join(path, fr["file_path"])
            if self.mode == "blender" and "." not in os.path.basename(fp):
                fp += ".png"
            poses.append(nerf_matrix_to_ngp(np.array(fr["transform_matrix"], dtype=np.float32), scale, offset))
            img = Image.open(fp)
            img = img.convert("RGBA" if img.mode in ("RGBA", "LA", "P") else "RGB")
            if H is None:
                W, H = img.size[0] // downscale, img.size[1] // downscale
            if img.size != (W, H):
                img = img.resize((W, H), Image.BOX)
            images.append(np.asarray(img, dtype=np.uint8) if store == "uint8"
                          else np.asarray(img, dtype=np.float32) / 255.0)
            if "dep_path" in fr:
                with np.load(os.path.join(path, fr["dep_path"])) as f:
                    depth = np.asarray(f["depth"], dtype=np.float32)
                if depth.ndim == 3 and depth.shape[-1] == 1:
                    depth = depth[..., 0]
                if depth.ndim != 2:
                    raise ValueError(f"NeRFDataset: {fr['dep_path']}: depth must be [H, W] or [H, W, 1], "
                                     f"got {list(depth.shape)}")
                if depth.shape != (H, W):
                    rows = np.minimum(np.floor(np.arange(H) * (depth.shape[0] / H)).astype(np.int64),
                                      depth.shape[0] - 1)
                    cols = np.minimum(np.floor(np.arange(W) * (depth.shape[1] / W)).astype(np.int64),
                                      depth.shape[1] - 1)
                    depth = depth[rows][:, cols]
                depths.append(depth)
            elif no_depth is None:
                no_depth = fr["file_path"]
        if depths and no_depth is not None:
            raise ValueError(f"NeRFDataset: frame {no_depth!r} has no dep_path, but other frames have one "
                             "(depth maps for every frame, or for none)")
        self.H, self.W = H, W
        self.depths = torch.from_numpy(np.ascontiguousarray(np.stack(depths))).to(device) if depths else None
        self.depth_scale = float(scale if depth_scale is None else depth_scale)
        self.error_map = (torch.ones(len(poses), self.error_map_res ** 2, dtype=torch.float32, device=device)
                          if error_map and type == "train" else None)
        self.poses = torch.from_numpy(np.stack(poses)).to(device)
        self.images = torch.from_numpy(np.stack(images)).to(device)
        # the uint8 store's divisor as a tensor: a true division on every device
        # (torch multiplies by the reciprocal when a GPU tensor is divided by a number)
        self._div = torch.full((1,), 255.0, device=device)
        if "fl_x" in transform or "fl_y" in transform:
            fl_x = (transform["fl_x"] if "fl_x" in transform else transform["fl_y"]) / downscale
            fl_y = (transform["fl_y"] if "fl_y" in transform else transform["fl_x"]) / downscale
        elif "camera_angle_x" in transform or "camera_angle_y" in transform:
            fl_x = W / (2 * math.tan(transform["camera_angle_x"] / 2)) if "camera_angle_x" in transform else None
            fl_y = H / (2 * math.tan(transform["camera_angle_y"] / 2)) if "camera_angle_y" in transform else None
            fl_x = fl_x if fl_x is not None else fl_y
            fl_y = fl_y if fl_y is not None else fl_x
        else:
            raise RuntimeError("NeRFDataset: no focal length (fl_x/fl_y or camera_angle_x/y) in the transforms")
        cx = transform["cx"] / downscale if "cx" in transform else W / 2
        cy = transform["cy"] / downscale if "cy" in transform else H / 2
        self.intrinsics = np.array([fl_x, fl_y, cx, cy], dtype=np.float32)
        self.radius = float(self.poses[:, :3, 3].norm(dim=-1).mean())

    def sample(self, index=None, generator=None):
        if index is None:
            index = int(torch.randint(0, self.poses.shape[0], (1,), generator=generator).item())
        poses = self.poses[index:index + 1]
        error_map = None if self.error_map is None else self.error_map[index:index + 1]
        rays = get_rays(poses, self.intrinsics, self.H, self.W, self.num_rays, error_map=error_map,
                        generator=generator)
        C = self.images.shape[-1]
        images = torch.gather(self.images[index:index + 1].view(1, -1, C), 1,
                              rays["inds"].unsqueeze(-1).expand(1, rays["inds"].shape[-1], C))
        if images.dtype == torch.uint8:
            images = images.float() / self._div
        out = {"H": self.H, "W": self.W, "rays_o": rays["rays_o"], "rays_d": rays["rays_d"], "images": images,
               "index": index}
        if "inds_coarse" in rays:
            out["inds_coarse"] = rays["inds_coarse"]  # the cells to fold the loss back into (utils.py:113)
        if self.depths is not None:
            # the same pixels' depths, in ngp units (one fp32 multiply, as the fused engine's gather)
            out["depths"] = torch.gather(self.depths[index:index + 1].view(1, -1), 1, rays["inds"]) * self.depth_scale
        return out
