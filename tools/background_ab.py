"""A/B of the fused step with and without a background model (--bg_radius) at
Config 2 on the image source (tools/image_source_ab.py's setup: 800 x 800, 100
poses, 4096 rays, Lego occupancy, a uint8 RGBA stack of the analytic target).

One build, one process: both trainers capture their multi-step graph and
settle, then `--repeats` interleaved rounds time `--steps` steps of each with
device events. The model-on trainer's launches are then timed one by one
(FusedTrainer.timed_body_steps: events between consecutive launches of eager
step bodies, a spin kernel ahead of each step), which gives the three added
launches' device times in the cache state of a real step. Writes a JSON.

    python tools/background_ab.py --out profiles/<tag>_background_ab.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--settle", type=int, default=512)
    ap.add_argument("--graph-steps", type=int, default=16)
    ap.add_argument("--num_rays", type=int, default=4096)
    ap.add_argument("--bg_radius", type=float, default=4.0)
    ap.add_argument("--kernel-steps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    from image_source_ab import ImageLego, render_stack
    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield

    dev = torch.device("cuda:0")
    lego = SyntheticLego(dev, num_rays=args.num_rays)
    data = ImageLego(lego, render_stack(lego))
    bits = torch.from_numpy(lego_bitfield()).to(dev)

    def model(radius):
        torch.manual_seed(0)
        m = NeRFNetwork(bound=1, cuda_ray=True, bg_radius=radius).to(dev)
        m.density_bitfield.copy_(bits)
        return m

    probe = FusedTrainer(model(-1), lego, M=args.num_rays * 64)
    counts = []
    for _ in range(4):
        probe.step()
        counts.append(probe.sample_count())
    M = int(np.mean(counts) * 1.25)
    del probe
    torch.cuda.empty_cache()

    trainers = {}
    for name, radius in (("off", -1), ("on", args.bg_radius)):
        ft = FusedTrainer(model(radius), data, M=M)
        for _ in range(5):
            ft.step()
        ft.capture(multi=args.graph_steps)
        trainers[name] = ft
    for _ in range(0, args.settle, 64):
        for ft in trainers.values():
            ft.run(64)
        torch.cuda.synchronize()

    ms = {name: [] for name in trainers}
    for _ in range(args.repeats):
        for name, ft in trainers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            ft.run(args.steps)
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / args.steps)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    launches = {}
    for name, ft in trainers.items():
        mean, per, _ = ft.timed_body_steps(args.kernel_steps)
        launches[name] = {k: {"mean_ms": float(v), "median_ms": float(np.median(per[k]))} for k, v in mean.items()}
    on = trainers["on"]
    result = {
        "config": {"H": lego.H, "W": lego.W, "n_poses": int(lego.poses.shape[0]), "num_rays": args.num_rays, "M": M,
                   "steps": args.steps, "repeats": args.repeats, "graph_steps": args.graph_steps,
                   "bg_radius": args.bg_radius, "kernel_steps": args.kernel_steps,
                   "background_parameters": int(on.params[3].numel() + on.params[4].numel()),
                   "device": torch.cuda.get_device_name(0)},
        "ms_per_step": ms,
        "median_ms_per_step": med,
        "spread_ms": {name: float(max(v) - min(v)) for name, v in ms.items()},
        "on_minus_off_ms": med["on"] - med["off"],
        "ratio_on_to_off": med["on"] / med["off"],
        "launch_ms": launches,
        "losses": {name: ft.last_loss for name, ft in trainers.items()},
        "device_errors": {name: ft.device_errors() for name, ft in trainers.items()},
    }
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
