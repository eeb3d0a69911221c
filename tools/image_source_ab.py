"""A/B of the fused step's batch source at Config 2 (800 x 800, 100 poses, 4096
rays, Lego occupancy): the analytic boxes (what bench.py measures) against the
image source with a uint8 and with a float32 RGBA stack. The stack is the
analytic target of every pixel, quantised on the device, so the three
trainers march the same scene with the same seed (the same rays; the targets
differ by the 1/255 rounding only).

One build, one process: each trainer captures its multi-step graph, all settle,
then `--repeats` interleaved rounds time `--steps` steps of each with device
events. Writes a JSON (per-source ms/step of every round, the medians, the
ratios to the analytic source).

    python tools/image_source_ab.py --out profiles/<tag>_image_source.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd")]


class ImageLego:
    """SyntheticLego's cameras with an image stack: what NeRFDataset hands the
    trainer (poses, intrinsics, H, W, num_rays, images)."""

    def __init__(self, lego, images):
        self.poses, self.intrinsics, self.H, self.W, self.num_rays = (lego.poses, lego.intrinsics, lego.H, lego.W,
                                                                       lego.num_rays)
        self.images = images


def render_stack(lego):
    """uint8 RGBA [n, H, W, 4] of SyntheticLego.target, one pose at a time."""
    from nerf.utils import get_rays
    out = torch.empty(lego.poses.shape[0], lego.H, lego.W, 4, dtype=torch.uint8, device=lego.poses.device)
    for k in range(lego.poses.shape[0]):
        rays = get_rays(lego.poses[k:k + 1], lego.intrinsics, lego.H, lego.W, -1)
        rgba = lego.target(rays["rays_o"], rays["rays_d"]).reshape(lego.H, lego.W, 4)
        out[k] = (rgba * 255).round().to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--settle", type=int, default=512)
    ap.add_argument("--graph-steps", type=int, default=16)
    ap.add_argument("--num_rays", type=int, default=4096)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield

    dev = torch.device("cuda:0")
    lego = SyntheticLego(dev, num_rays=args.num_rays)
    u8 = render_stack(lego)
    f32 = u8.float() / torch.full((1,), 255.0, device=dev)
    bits = torch.from_numpy(lego_bitfield()).to(dev)

    def model():
        torch.manual_seed(0)
        m = NeRFNetwork(bound=1, cuda_ray=True).to(dev)
        m.density_bitfield.copy_(bits)
        return m

    # the sample buffer as bench.py sizes it: 1.25 x the measured mean count
    probe = FusedTrainer(model(), lego, M=args.num_rays * 64)
    counts = []
    for _ in range(4):
        probe.step()
        counts.append(probe.sample_count())
    M = int(np.mean(counts) * 1.25)
    del probe
    torch.cuda.empty_cache()

    sources = {"analytic": lego, "image_uint8": ImageLego(lego, u8), "image_float32": ImageLego(lego, f32)}
    trainers = {}
    for name, data in sources.items():
        ft = FusedTrainer(model(), data, M=M)
        for _ in range(5):
            ft.step()
        ft.capture(multi=args.graph_steps)
        trainers[name] = ft
    for i in range(0, args.settle, 64):
        for ft in trainers.values():
            ft.run(64)
        torch.cuda.synchronize()

    ms = {name: [] for name in trainers}
    samples = {name: [] for name in trainers}
    for _ in range(args.repeats):
        for name, ft in trainers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            ft.run(args.steps)
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / args.steps)
            samples[name].append(ft.sample_count())
    med = {name: float(np.median(v)) for name, v in ms.items()}
    result = {
        "config": {"H": lego.H, "W": lego.W, "n_poses": int(lego.poses.shape[0]), "num_rays": args.num_rays, "M": M,
                   "steps": args.steps, "repeats": args.repeats, "graph_steps": args.graph_steps,
                   "stack_MiB": {"uint8": u8.numel() / 2 ** 20, "float32": f32.numel() * 4 / 2 ** 20},
                   "device": torch.cuda.get_device_name(0)},
        "ms_per_step": ms,
        "median_ms_per_step": med,
        "rays_per_s": {name: args.num_rays / (v * 1e-3) for name, v in med.items()},
        "spread_ms": {name: float(max(v) - min(v)) for name, v in ms.items()},
        "ratio_to_analytic": {name: med[name] / med["analytic"] for name in med},
        "last_sample_counts": samples,
        "losses": {name: ft.last_loss for name, ft in trainers.items()},
        "device_errors": {name: ft.device_errors() for name, ft in trainers.items()},
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
