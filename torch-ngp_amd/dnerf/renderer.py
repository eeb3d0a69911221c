"""D-NeRF renderer (reference dnerf/renderer.py:61-591): the static renderer
with one occupancy grid per time slice, `density_grid` [T, C, H^3] and
`density_bitfield` [T, C * H^3 / 8]. A ray batch has one time; it is marched
through the bitfield of slice floor(time * T) by the existing raymarching
operators, which take the slice as the bitfield they already accept.

update_extra_state is the reference's :454-555 in three device steps
(csrc/dnerf.hip) instead of Python loops over 64 slices x
cascades x blocks with a nonzero() read-back each: the query points of a chunk
(ngp_dnerf_grid_points), their densities from the network in torch, scattered
as a max into the scratch grid, and one EMA + global mean + pack over every
slice (ngp_dnerf_grid_ema_pack). The host reads back stats[0] and mean_count,
nothing else. Deliberate differences from the reference: the time jitter is
drawn per point (the reference draws one per block: the same distribution),
the draws come from the counter RNG (`grid_seed`, the update's number), a
segment without occupied cells draws its second half uniformly (the reference
would raise), and a cell drawn twice keeps the larger density.

Only the cuda_ray path exists (the reference's run() is not included)."""
import math

import numpy as np
import torch
import torch.nn as nn

import raymarching

from . import backend


def custom_meshgrid(*args):
    return torch.meshgrid(*args, indexing="ij")


class NeRFRenderer(nn.Module):
    def __init__(self, bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=0.01, bg_radius=-1,
                 time_size=64, grid_size=128):
        super().__init__()
        if not cuda_ray:
            raise NotImplementedError("dnerf: only the cuda_ray path is included")
        if bg_radius > 0:
            raise NotImplementedError("dnerf: the background model (bg_radius > 0) is not included")
        if not (isinstance(time_size, int) and 1 <= time_size <= 1024):
            raise ValueError(f"time_size must be an integer in [1, 1024], got {time_size!r}")
        if not (isinstance(grid_size, int) and 2 <= grid_size <= 1024 and grid_size & (grid_size - 1) == 0):
            raise ValueError(f"grid_size must be a power of two in [2, 1024], got {grid_size!r}")
        self.bound = bound
        self.cascade = 1 + math.ceil(math.log2(bound))
        self.time_size = time_size
        self.grid_size = grid_size
        self.density_scale = density_scale
        self.min_near = min_near
        self.density_thresh = density_thresh
        self.bg_radius = bg_radius
        self.grid_seed = 0  # the counter RNG's seed of the grid updates

        aabb_train = torch.FloatTensor([-bound, -bound, -bound, bound, bound, bound])
        self.register_buffer("aabb_train", aabb_train)
        self.register_buffer("aabb_infer", aabb_train.clone())

        self.cuda_ray = cuda_ray
        T, C, H3 = time_size, self.cascade, grid_size ** 3
        self.register_buffer("density_grid", torch.zeros(T, C, H3))
        self.register_buffer("density_bitfield", torch.zeros(T, C * H3 // 8, dtype=torch.uint8))
        self.mean_density = 0
        self.iter_density = 0
        self.register_buffer("times", ((torch.arange(T, dtype=torch.float32) + 0.5) / T).view(-1, 1, 1))
        self.register_buffer("step_counter", torch.zeros(16, 2, dtype=torch.int32))
        self.mean_count = 0
        self.local_step = 0

    def forward(self, x, d, t):
        raise NotImplementedError()

    def density(self, x, t):
        raise NotImplementedError()

    def color(self, x, d, mask=None, **kwargs):
        raise NotImplementedError()

    def reset_extra_state(self):
        self.density_grid.zero_()
        self.mean_density = 0
        self.iter_density = 0
        self.step_counter.zero_()
        self.mean_count = 0
        self.local_step = 0

    def time_slice(self, time):
        """The grid slice of a batch's time [B, 1] (its first entry): floor(time * T) in [0, T - 1]."""
        return torch.floor(time[0][0] * self.time_size).clamp(min=0, max=self.time_size - 1).long()

    def run_cuda(self, rays_o, rays_d, time, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False,
                 max_steps=1024, T_thresh=1e-4, **kwargs):
        """rays_o, rays_d [B, N, 3] (B = 1), time [B, 1] -> image [B, N, 3], depth [B, N] (:261-386)."""
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        N = rays_o.shape[0]
        device = rays_o.device
        nears, fars = raymarching.near_far_from_aabb(
            rays_o, rays_d, self.aabb_train if self.training else self.aabb_infer, self.min_near)
        if bg_color is None:
            bg_color = 1
        bitfield = self.density_bitfield[self.time_slice(time)]
        results = {}
        if self.training:
            counter = self.step_counter[self.local_step % 16]
            counter.zero_()
            self.local_step += 1
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(
                rays_o, rays_d, self.bound, bitfield, self.cascade, self.grid_size, nears, fars, counter,
                self.mean_count, perturb, 128, force_all_rays, dt_gamma, max_steps)
            sigmas, rgbs, deform = self(xyzs, dirs, time)
            sigmas = self.density_scale * sigmas
            weights_sum, depth, image = raymarching.composite_rays_train(sigmas, rgbs, deltas, rays, T_thresh)
            image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
            depth = torch.clamp(depth - nears, min=0) / (fars - nears)
            results["deform"] = deform
        else:
            weights_sum = torch.zeros(N, dtype=torch.float32, device=device)
            depth = torch.zeros(N, dtype=torch.float32, device=device)
            image = torch.zeros(N, 3, dtype=torch.float32, device=device)
            rays_alive = torch.arange(N, dtype=torch.int32, device=device)
            rays_t = nears.clone()
            step = 0
            while step < max_steps:
                n_alive = rays_alive.shape[0]
                if n_alive <= 0:
                    break
                n_step = max(min(N // n_alive, 8), 1)
                xyzs, dirs, deltas = raymarching.march_rays(
                    n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound, bitfield, self.cascade,
                    self.grid_size, nears, fars, 128, perturb if step == 0 else False, dt_gamma, max_steps)
                sigmas, rgbs, _ = self(xyzs, dirs, time)
                sigmas = self.density_scale * sigmas
                raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum,
                                           depth, image, T_thresh)
                rays_alive = rays_alive[rays_alive >= 0]
                step += n_step
            image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
            depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        results["depth"] = depth.view(*prefix)
        results["image"] = image.view(*prefix, 3)
        return results

    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsic, S=64):
        """Cells no training camera sees become -1 in every slice (:389-451):
        one count per cascade, applied to all T slices."""
        if isinstance(poses, np.ndarray):
            poses = torch.from_numpy(poses)
        B = poses.shape[0]
        fx, fy, cx, cy = intrinsic
        dev = self.density_bitfield.device
        X = torch.arange(self.grid_size, dtype=torch.int32, device=dev).split(S)
        count = torch.zeros_like(self.density_grid[0])
        poses = poses.to(dev)
        for xs in X:
            for ys in X:
                for zs in X:
                    xx, yy, zz = custom_meshgrid(xs, ys, zs)
                    coords = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
                    indices = raymarching.morton3D(coords).long()
                    world = (2 * coords.float() / (self.grid_size - 1) - 1).unsqueeze(0)
                    for cas in range(self.cascade):
                        bound = min(2 ** cas, self.bound)
                        hgs = bound / self.grid_size
                        cas_world = world * (bound - hgs)
                        head = 0
                        while head < B:
                            tail = min(head + S, B)
                            cam = cas_world - poses[head:tail, :3, 3].unsqueeze(1)
                            cam = cam @ poses[head:tail, :3, :3]
                            mz = cam[:, :, 2] > 0
                            mx = torch.abs(cam[:, :, 0]) < cx / fx * cam[:, :, 2] + hgs * 2
                            my = torch.abs(cam[:, :, 1]) < cy / fy * cam[:, :, 2] + hgs * 2
                            count[cas, indices] += (mz & mx & my).sum(0).reshape(-1)
                            head += S
        self.density_grid[(count == 0).unsqueeze(0).expand_as(self.density_grid)] = -1

    def _density_tmp(self):
        """The update's scratch grid (-1 = not queried); the EMA pass resets it."""
        t = getattr(self, "_tmp_grid", None)
        if t is None or t.shape != self.density_grid.shape or t.device != self.density_grid.device:
            t = torch.full_like(self.density_grid, -1.0)
            self._tmp_grid = t
        return t

    def update_chunks(self):
        """(partial, [(lo, hi), ...]) of the next update: every cell while
        iter_density < 16, the partial draw while < 100, nothing after; at
        most C * H^3 points per query."""
        T, C, H3 = self.time_size, self.cascade, self.grid_size ** 3
        if self.iter_density < 16:
            partial, P = False, T * C * H3
        elif self.iter_density < 100:
            partial, P = True, T * C * 2 * (H3 // 4)
        else:
            return False, []
        step = C * H3
        return partial, [(lo, min(lo + step, P)) for lo in range(0, P, step)]

    @torch.no_grad()
    def update_extra_state(self, decay=0.95):
        T, C, H = self.time_size, self.cascade, self.grid_size
        tmp = self._density_tmp()
        partial, chunks = self.update_chunks()
        ws = None
        if partial:
            ws = getattr(self, "_points_ws", None)
            if ws is None or ws.device != tmp.device:
                ws = self._points_ws = backend.grid_points_workspace(T, C, H, tmp.device)
        flat = tmp.view(-1)
        for lo, hi in chunks:
            xyzs, times, indices = backend.grid_points(self.density_grid, T, C, H, self.bound, partial,
                                                       self.grid_seed, self.iter_density, lo, hi, ws)
            sigmas = self.density(xyzs, times.unsqueeze(-1))["sigma"].reshape(-1).detach().float()
            sigmas = sigmas * self.density_scale
            if partial:  # a cell drawn twice keeps the larger density (sigma >= 0: the bits order as the values)
                flat.view(torch.int32).scatter_reduce_(0, indices.long(), sigmas.view(torch.int32), "amax")
            else:  # row = cell
                flat[lo:hi] = sigmas
        stats = backend.grid_ema_pack(self.density_grid, tmp, T, C, H, decay, self.density_thresh,
                                      self.density_bitfield)
        self.mean_density = float(np.float32(stats[0].item() / self.density_grid.numel()))
        self.iter_density += 1
        total_step = min(16, self.local_step)
        if total_step > 0:
            self.mean_count = int(self.step_counter[:total_step, 0].sum().item() / total_step)
        self.local_step = 0

    def render(self, rays_o, rays_d, time, staged=False, max_ray_batch=4096, **kwargs):
        """rays_o, rays_d [B, N, 3], time [B, 1] -> {'image' [B, N, 3], 'depth' [B, N]}; never staged (cuda_ray)."""
        return self.run_cuda(rays_o, rays_d, time, **kwargs)
