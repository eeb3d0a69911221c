"""NeRF renderer: the hot-path caller (reference nerf/renderer.py:62-634).

Restores the upstream torch-ngp behaviour the research fork broke (SURVEY
§1.3): density grid updates work (update_extra_state), no Minkowski /
frnn branches in run_cuda, no trimesh import. Public methods and buffers
(`density_grid`, `density_bitfield`, `step_counter`, `mean_count`, ...) keep
the reference names so checkpoints and trainers interoperate.
"""
import math

import numpy as np
import torch
import torch.nn as nn

import raymarching


def custom_meshgrid(*args):
    return torch.meshgrid(*args, indexing="ij")


def sample_pdf(bins, weights, n_samples, det=False):
    """Inverse-CDF sampling (reference renderer.py:12-46)."""
    weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    if det:
        u = torch.linspace(0.5 / n_samples, 1.0 - 0.5 / n_samples, steps=n_samples, device=weights.device)
        u = u.expand(list(cdf.shape[:-1]) + [n_samples])
    else:
        u = torch.rand(list(cdf.shape[:-1]) + [n_samples], device=weights.device)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    inds_g = torch.stack([below, above], -1)
    shape = [inds_g.shape[0], inds_g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(shape), 2, inds_g)
    bins_g = torch.gather(bins.unsqueeze(1).expand(shape), 2, inds_g)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    return bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])


class NeRFRenderer(nn.Module):
    def __init__(self, bound=1, cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01,
                 bg_radius=-1, grid_size=128, **kwargs):
        super().__init__()
        self.bound = bound
        self.cascade = 1 + math.ceil(math.log2(bound))
        # a cell's index is its Morton code: below grid_size^3 only for a power of two
        if not (isinstance(grid_size, int) and 2 <= grid_size <= 1024 and grid_size & (grid_size - 1) == 0):
            raise ValueError(f"grid_size must be a power of two in [2, 1024], got {grid_size!r}")
        self.grid_size = grid_size
        self.density_scale = density_scale
        self.min_near = min_near
        self.density_thresh = density_thresh
        self.bg_radius = bg_radius

        aabb_train = torch.FloatTensor([-bound, -bound, -bound, bound, bound, bound])
        self.register_buffer("aabb_train", aabb_train)
        self.register_buffer("aabb_infer", aabb_train.clone())

        self.cuda_ray = cuda_ray
        if cuda_ray:
            self.register_buffer("density_grid", torch.zeros([self.cascade, grid_size ** 3]))
            self.register_buffer("density_bitfield",
                                 torch.zeros(self.cascade * grid_size ** 3 // 8, dtype=torch.uint8))
            self.mean_density = 0
            self.iter_density = 0
            self.register_buffer("step_counter", torch.zeros(16, 2, dtype=torch.int32))
            self.mean_count = 0
            self.local_step = 0

    def forward(self, x, d):
        raise NotImplementedError()

    def density(self, x):
        raise NotImplementedError()

    def color(self, x, d, mask=None, **kwargs):
        raise NotImplementedError()

    def background(self, x, d):
        raise NotImplementedError()

    def reset_extra_state(self):
        if not self.cuda_ray:
            return
        self.density_grid.zero_()
        self.mean_density = 0
        self.iter_density = 0
        self.step_counter.zero_()
        self.mean_count = 0
        self.local_step = 0

    # ------------------------------------------------------------- torch path
    def run(self, rays_o, rays_d, num_steps=128, upsample_steps=128, bg_color=None, perturb=False,
            **kwargs):
        """Uniform (+ importance) sampling without the density grid (renderer.py:126-254)."""
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        N = rays_o.shape[0]
        device = rays_o.device
        aabb = self.aabb_train if self.training else self.aabb_infer
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        nears, fars = nears.unsqueeze(-1), fars.unsqueeze(-1)

        z_vals = torch.linspace(0.0, 1.0, num_steps, device=device).unsqueeze(0).expand(N, num_steps)
        z_vals = nears + (fars - nears) * z_vals
        sample_dist = (fars - nears) / num_steps
        if perturb:
            z_vals = z_vals + (torch.rand(z_vals.shape, device=device) - 0.5) * sample_dist
        xyzs = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z_vals.unsqueeze(-1)
        xyzs = torch.min(torch.max(xyzs, aabb[:3]), aabb[3:])
        dens = {k: v.view(N, num_steps, -1) for k, v in self.density(xyzs.reshape(-1, 3)).items()}

        if upsample_steps > 0:
            with torch.no_grad():
                deltas = z_vals[..., 1:] - z_vals[..., :-1]
                deltas = torch.cat([deltas, sample_dist * torch.ones_like(deltas[..., :1])], dim=-1)
                alphas = 1 - torch.exp(-deltas * self.density_scale * dens["sigma"].squeeze(-1))
                alphas_shifted = torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15], dim=-1)
                weights = alphas * torch.cumprod(alphas_shifted, dim=-1)[..., :-1]
                z_mid = z_vals[..., :-1] + 0.5 * deltas[..., :-1]
                new_z = sample_pdf(z_mid, weights[:, 1:-1], upsample_steps, det=not self.training).detach()
                new_xyzs = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * new_z.unsqueeze(-1)
                new_xyzs = torch.min(torch.max(new_xyzs, aabb[:3]), aabb[3:])
            new_dens = {k: v.view(N, upsample_steps, -1)
                        for k, v in self.density(new_xyzs.reshape(-1, 3)).items()}
            z_vals, z_index = torch.sort(torch.cat([z_vals, new_z], dim=1), dim=1)
            xyzs = torch.cat([xyzs, new_xyzs], dim=1)
            xyzs = torch.gather(xyzs, 1, z_index.unsqueeze(-1).expand_as(xyzs))
            for k in dens:
                tmp = torch.cat([dens[k], new_dens[k]], dim=1)
                dens[k] = torch.gather(tmp, 1, z_index.unsqueeze(-1).expand_as(tmp))

        deltas = z_vals[..., 1:] - z_vals[..., :-1]
        deltas = torch.cat([deltas, sample_dist * torch.ones_like(deltas[..., :1])], dim=-1)
        alphas = 1 - torch.exp(-deltas * self.density_scale * dens["sigma"].squeeze(-1))
        alphas_shifted = torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15], dim=-1)
        weights = alphas * torch.cumprod(alphas_shifted, dim=-1)[..., :-1]
        dirs = rays_d.view(-1, 1, 3).expand_as(xyzs)
        dens = {k: v.reshape(-1, v.shape[-1]) for k, v in dens.items()}
        mask = weights > 1e-4
        rgbs = self.color(xyzs.reshape(-1, 3), dirs.reshape(-1, 3), mask=mask.reshape(-1), **dens)
        rgbs = rgbs.view(N, -1, 3)
        weights_sum = weights.sum(dim=-1)
        ori_z = ((z_vals - nears) / (fars - nears)).clamp(0, 1)
        depth = torch.sum(weights * ori_z, dim=-1)
        image = torch.sum(weights.unsqueeze(-1) * rgbs, dim=-2)
        if self.bg_radius > 0:
            sph = raymarching.sph_from_ray(rays_o, rays_d, self.bg_radius)
            bg_color = self.background(sph, rays_d.reshape(-1, 3))
        elif bg_color is None:
            bg_color = 1
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3),
                "weights_sum": weights_sum}

    # -------------------------------------------------------------- HIP path
    def run_cuda(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False,
                 force_all_rays=False, max_steps=1024, T_thresh=1e-4, dist_loss=False, **kwargs):
        """Density-grid ray marching (renderer.py:257-431, upstream semantics).
        dist_loss (training mode): also results["distortion"], each ray's
        distortion term (raymarching.distortion_rays_train)."""
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        N = rays_o.shape[0]
        device = rays_o.device

        nears, fars = raymarching.near_far_from_aabb(
            rays_o, rays_d, self.aabb_train if self.training else self.aabb_infer, self.min_near)

        if self.bg_radius > 0:
            sph = raymarching.sph_from_ray(rays_o, rays_d, self.bg_radius)
            bg_color = self.background(sph, rays_d)
        elif bg_color is None:
            bg_color = 1

        results = {}
        if self.training:
            counter = self.step_counter[self.local_step % 16]
            counter.zero_()
            self.local_step += 1
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(
                rays_o, rays_d, self.bound, self.density_bitfield, self.cascade, self.grid_size,
                nears, fars, counter, self.mean_count, perturb, 128, force_all_rays, dt_gamma,
                max_steps)
            sigmas, rgbs = self(xyzs, dirs)
            sigmas = self.density_scale * sigmas
            weights_sum, depth, image = raymarching.composite_rays_train(sigmas, rgbs, deltas, rays,
                                                                         T_thresh)
            if dist_loss:
                results["distortion"] = raymarching.distortion_rays_train(sigmas, deltas, rays, T_thresh)
            image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
            # the composite's depth in ngp units, what depth supervision compares (renderer.py:369)
            results["depth_bound_scale"] = torch.clamp(depth, min=0).view(*prefix)
            depth = torch.clamp(depth - nears, min=0) / (fars - nears)
            results["weights_sum"] = weights_sum
            image = image.view(*prefix, 3)
            depth = depth.view(*prefix)
        else:
            dtype = torch.float32
            weights_sum = torch.zeros(N, dtype=dtype, device=device)
            depth = torch.zeros(N, dtype=dtype, device=device)
            image = torch.zeros(N, 3, dtype=dtype, device=device)
            rays_alive = torch.arange(N, dtype=torch.int32, device=device)
            rays_t = nears.clone()
            step = 0
            while step < max_steps:
                n_alive = rays_alive.shape[0]
                if n_alive <= 0:
                    break
                n_step = max(min(N // n_alive, 8), 1)
                xyzs, dirs, deltas = raymarching.march_rays(
                    n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound,
                    self.density_bitfield, self.cascade, self.grid_size, nears, fars, 128,
                    perturb if step == 0 else False, dt_gamma, max_steps)
                sigmas, rgbs = self(xyzs, dirs)
                sigmas = self.density_scale * sigmas
                raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas,
                                           weights_sum, depth, image, T_thresh)
                rays_alive = rays_alive[rays_alive >= 0]
                step += n_step
            image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
            depth = torch.clamp(depth - nears, min=0) / (fars - nears)
            image = image.view(*prefix, 3)
            depth = depth.view(*prefix)
        results["depth"] = depth
        results["image"] = image
        return results

    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsic, S=64):
        """Mark cells no training camera sees as -1 (renderer.py:433-496)."""
        if not self.cuda_ray:
            return
        if isinstance(poses, np.ndarray):
            poses = torch.from_numpy(poses)
        B = poses.shape[0]
        fx, fy, cx, cy = intrinsic
        dev = self.density_bitfield.device
        X = torch.arange(self.grid_size, dtype=torch.int32, device=dev).split(S)
        count = torch.zeros_like(self.density_grid)
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
        self.density_grid[count == 0] = -1

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=128):
        """EMA density-grid update + packbits + mean_count (renderer.py:498-598,
        upstream cadence: every update_extra_interval steps).

        The random draws are the reference's torch ones in its order (per
        block and cascade: rand_like noise; partial updates: randint cells,
        nonzero + randint occupied cells), so an update consumes the torch RNG
        exactly as upstream. Everything after them runs on the device without a
        host round trip (csrc/density_grid.hip): query points, their densities
        (`_query_density`), the EMA, the mean and the bitfield. A cell drawn
        twice in one partial update keeps the larger density (upstream keeps
        an arbitrary one of them)."""
        if not self.cuda_ray:
            return
        import _ngp_native as nat
        dev = self.density_bitfield.device
        H, C = self.grid_size, self.cascade
        if self.iter_density < 16:
            X = torch.arange(H, dtype=torch.int32, device=dev).split(S)
            blocks = [(xs, ys, zs) for xs in X for ys in X for zs in X]
            noise = [[None] * len(blocks) for _ in range(C)]
            for bi, (xs, ys, zs) in enumerate(blocks):
                n = len(xs) * len(ys) * len(zs)
                for cas in range(C):  # rand_like(cas_xyzs), :533
                    noise[cas][bi] = torch.rand(n, 3, device=dev)
            if len(blocks) == 1:
                coords = None  # every cell, meshgrid order
            else:
                cb = []
                for xs, ys, zs in blocks:
                    xx, yy, zz = custom_meshgrid(xs, ys, zs)
                    cb.append(torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1))
                coords = torch.cat(cb).repeat(C, 1).contiguous()
            noise = torch.cat([torch.cat(nc) for nc in noise]).contiguous()
            ppc = H ** 3
        else:
            N = H ** 3 // 4
            cs, ns = [], []
            for cas in range(C):  # :551-569
                coords = torch.randint(0, H, (N, 3), device=dev)
                occ = torch.nonzero(self.density_grid[cas] > 0).squeeze(-1)
                rand_mask = torch.randint(0, max(occ.shape[0], 1), [N], dtype=torch.long, device=dev)
                occ_coords = (raymarching.morton3D_invert(occ[rand_mask].int()) if occ.shape[0] > 0
                              else coords.int())
                cc = torch.cat([coords.int(), occ_coords], dim=0)
                cs.append(cc)
                ns.append(torch.rand(cc.shape, device=dev))
            coords = torch.cat(cs).contiguous()
            noise = torch.cat(ns).contiguous()
            ppc = 2 * N
        P = ppc * C
        xyzs = torch.empty(P, 3, device=dev)
        indices = torch.empty(P, dtype=torch.int32, device=dev)
        st = nat.stream_of(xyzs)
        nat.check(nat.lib().ngp_density_grid_points(nat.ptr(coords), nat.ptr(noise), P, ppc, C, H,
                                                    float(self.bound), nat.ptr(xyzs), nat.ptr(indices), st),
                  "density_grid_points")
        tmp = self._density_tmp()
        # one cascade's worth of points per query at most (the reference queries
        # one block of one cascade at a time, :535): the scatter-max into tmp is
        # order-independent, so the slices give the same grid
        step = H ** 3
        for a in range(0, P, step):
            self._query_density(xyzs[a:a + step], indices[a:a + step], tmp)
        stats = torch.empty(nat.DENSITY_STATS_LEN, dtype=torch.float64, device=dev)
        nat.check(nat.lib().ngp_density_grid_ema_pack(nat.ptr(self.density_grid), nat.ptr(tmp), C, H,
                                                      float(decay), float(self.density_thresh), nat.ptr(stats),
                                                      nat.ptr(self.density_bitfield), st),
                  "density_grid_ema_pack")
        # mean_density: torch.mean(...).item() of the fp32 grid, :584
        self.mean_density = float(np.float32(stats[0].item() / self.density_grid.numel()))
        self.iter_density += 1
        total_step = min(16, self.local_step)
        if total_step > 0:
            self.mean_count = int(self.step_counter[:total_step, 0].sum().item() / total_step)
        self.local_step = 0

    def _density_tmp(self):
        """The update's scratch grid (-1 = not queried); the EMA pass resets it."""
        t = getattr(self, "_tmp_grid", None)
        if t is None or t.shape != self.density_grid.shape or t.device != self.density_grid.device:
            t = torch.full_like(self.density_grid, -1.0)
            self._tmp_grid = t
        return t

    def _query_density(self, xyzs, indices, tmp_grid):
        """tmp_grid[indices] = max(.., density(xyzs) * density_scale)
        (renderer.py:535-538). Networks with a fused density kernel override it."""
        sigmas = self.density(xyzs)["sigma"].reshape(-1).detach().float() * self.density_scale
        tmp_grid.view(-1).view(torch.int32).scatter_reduce_(0, indices.long(), sigmas.view(torch.int32), "amax")

    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """rays_o/rays_d [B, N, 3] -> {'image' [B, N, 3], 'depth' [B, N], ...}."""
        _run = self.run_cuda if self.cuda_ray else self.run
        B, N = rays_o.shape[:2]
        device = rays_o.device
        if staged and not self.cuda_ray:
            depth = torch.empty((B, N), device=device)
            image = torch.empty((B, N, 3), device=device)
            for b in range(B):
                head = 0
                while head < N:
                    tail = min(head + max_ray_batch, N)
                    r = _run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], **kwargs)
                    depth[b:b + 1, head:tail] = r["depth"]
                    image[b:b + 1, head:tail] = r["image"]
                    head += max_ray_batch
            return {"depth": depth, "image": image}
        return _run(rays_o, rays_d, **kwargs)
