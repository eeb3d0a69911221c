"""Times D-NeRF's time-sliced density-grid update on the GPU
at the reference's shape, T = 64 slices, H = 128, bound = 2 (2 cascades: the
grid and its scratch are 1 GiB each):

  full_device / partial_device    NeRFRenderer.update_extra_state: the three
                                  device steps of csrc/dnerf.hip around the
                                  network's density query in torch
  full_torch / partial_torch      a torch restatement of the reference's loops
                                  (dnerf/renderer.py:454-555: per slice, cascade
                                  and block in Python, nonzero() and randint per
                                  slice and cascade, one packbits per slice, a
                                  global mean) with the same network
  step                            one DNeRFTrainer.train_step (4096 rays of the
                                  analytic Lego solid at a random frame time,
                                  no grid update)

Both update paths run the same NeRFNetwork.density under fp16 autocast, so the
difference between them is everything around the network. Every figure is the
median of `--repeats` interleaved rounds after `--warmup` untimed ones, device
events around each call. No GPU: an error, never a CPU figure.

usage: python tools/dnerf_bench.py [--out profiles/dnerf_bench.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd"), HERE]

import torch  # noqa: E402

from sdf_bench import interleaved  # noqa: E402


@torch.no_grad()
def reference_update(m, decay=0.95, S=128):
    """The reference's update_extra_state (dnerf/renderer.py:454-555) in torch, on the model's buffers."""
    import raymarching
    dev = m.density_bitfield.device
    H = m.grid_size
    tmp_grid = -torch.ones_like(m.density_grid)
    hts = 0.5 / m.time_size
    if m.iter_density < 16:
        X = torch.arange(H, dtype=torch.int32, device=dev).split(S)
        for t, time in enumerate(m.times):
            for xs in X:
                for ys in X:
                    for zs in X:
                        xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                        coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                        indices = raymarching.morton3D(coords).long()
                        xyzs = 2 * coords.float() / (H - 1) - 1
                        for cas in range(m.cascade):
                            bound = min(2 ** cas, m.bound)
                            hgs = bound / H
                            cas_xyzs = xyzs * (bound - hgs)
                            cas_xyzs += (torch.rand_like(cas_xyzs) * 2 - 1) * hgs
                            time_perturb = time + (torch.rand_like(time) * 2 - 1) * hts
                            sigmas = m.density(cas_xyzs, time_perturb)["sigma"].reshape(-1).detach().float()
                            sigmas *= m.density_scale
                            tmp_grid[t, cas, indices] = sigmas
    elif m.iter_density < 100:
        N = H ** 3 // 4
        for t, time in enumerate(m.times):
            for cas in range(m.cascade):
                coords = torch.randint(0, H, (N, 3), device=dev)
                indices = raymarching.morton3D(coords.int()).long()
                occ_indices = torch.nonzero(m.density_grid[t, cas] > 0).squeeze(-1)
                rand_mask = torch.randint(0, occ_indices.shape[0], [N], dtype=torch.long, device=dev)
                occ_indices = occ_indices[rand_mask]
                occ_coords = raymarching.morton3D_invert(occ_indices.int())
                indices = torch.cat([indices, occ_indices], dim=0)
                coords = torch.cat([coords, occ_coords], dim=0)
                xyzs = 2 * coords.float() / (H - 1) - 1
                bound = min(2 ** cas, m.bound)
                hgs = bound / H
                cas_xyzs = xyzs * (bound - hgs)
                cas_xyzs += (torch.rand_like(cas_xyzs) * 2 - 1) * hgs
                time_perturb = time + (torch.rand_like(time) * 2 - 1) * hts
                sigmas = m.density(cas_xyzs, time_perturb)["sigma"].reshape(-1).detach().float()
                sigmas *= m.density_scale
                tmp_grid[t, cas, indices] = sigmas
    valid = (m.density_grid >= 0) & (tmp_grid >= 0)
    m.density_grid[valid] = torch.maximum(m.density_grid[valid] * decay, tmp_grid[valid])
    m.mean_density = torch.mean(m.density_grid.clamp(min=0)).item()
    m.iter_density += 1
    thresh = min(m.mean_density, m.density_thresh)
    for t in range(m.time_size):
        raymarching.packbits(m.density_grid[t], thresh, m.density_bitfield[t])
    total_step = min(16, m.local_step)
    if total_step > 0:
        m.mean_count = int(m.step_counter[:total_step, 0].sum().item() / total_step)
    m.local_step = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time_size", type=int, default=64)
    ap.add_argument("--grid_size", type=int, default=128)
    ap.add_argument("--bound", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step_inner", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "dnerf_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dnerf_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from dnerf import DNeRFTrainer, NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield

    torch.manual_seed(0)
    model = NeRFNetwork(bound=args.bound, time_size=args.time_size, grid_size=args.grid_size,
                        density_thresh=10).to(dev)
    model.train()
    T, C, H = model.time_size, model.cascade, model.grid_size

    def update(fn, iter_density):
        def run():
            model.iter_density = iter_density
            with torch.autocast("cuda", dtype=torch.float16):
                fn()
        return run

    variants = {"full_device": update(model.update_extra_state, 0),
                "full_torch": update(lambda: reference_update(model), 0),
                "partial_device": update(model.update_extra_state, 16),
                "partial_torch": update(lambda: reference_update(model), 16)}
    res = {"device": torch.cuda.get_device_name(0), "time_size": T, "cascade": C, "grid_size": H,
           "points_full": T * C * H ** 3, "points_partial": T * C * 2 * (H ** 3 // 4),
           "method": f"median of {args.repeats} interleaved rounds after {args.warmup} warm-up round(s); device "
                     "events around one update (a step: around --step_inner steps); the same network under fp16 "
                     "autocast on both paths"}
    res.update(interleaved(variants, args.warmup, args.repeats, 1))
    for kind in ("full", "partial"):
        res[f"{kind}_torch_over_device"] = round(res[f"{kind}_torch"]["median_ms"] /
                                                 res[f"{kind}_device"]["median_ms"], 3)

    # one training step: the Lego solid's rays at a random frame time, its occupancy in every slice
    class TimedLego(SyntheticLego):
        def sample(self, index=None):
            out = super().sample(index)
            out["time"] = torch.rand(1, 1, device=self.device)
            return out

    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield(C, H, float(args.bound))).to(dev)[None].expand(T, -1))
    trainer = DNeRFTrainer(model, TimedLego(dev, num_rays=4096),
                           iters=30000, update_extra_interval=10 ** 9, dt_gamma=1 / 128 if args.bound > 1 else 0,
                           log=None)
    trainer.global_step = 1  # (no grid update: the Lego occupancy stays)
    for _ in range(3):
        trainer.train_step()
    k = min(16, model.local_step)
    model.mean_count = int(model.step_counter[:k, 0].sum().item() / k)  # as update_extra_state sets it
    res.update(interleaved({"step": trainer.train_step}, max(args.warmup, 2), max(args.repeats, 5), args.step_inner))
    res["step_num_rays"], res["step_samples"] = 4096, model.mean_count
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
