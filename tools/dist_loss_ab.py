"""A/B of the distortion regulariser (FusedTrainer(dist_loss_weight=W)) on the
Lego bench shape (800 x 800, 100 poses, 4096 rays, Lego occupancy, the sample
buffer sized as bench.py sizes it), by the method of tools/error_map_ab.py: the
term off against on, the same model, seed and sample buffer. One build, one
process: each trainer captures its multi-step graph, both settle, then
`--repeats` interleaved rounds time `--steps` steps of each with device events;
the composite launch's own time is the step body's per-launch time as the
graphs run it (timed_body_steps), with the share of live rows of those steps.
Reported, not gated. Writes a JSON.

    python tools/dist_loss_ab.py --out profiles/<tag>_dist_loss.json
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
    ap.add_argument("--weight", type=float, default=0.01)
    ap.add_argument("--body-steps", type=int, default=32)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield

    dev = torch.device("cuda:0")
    lego = SyntheticLego(dev, num_rays=args.num_rays)
    bits = torch.from_numpy(lego_bitfield()).to(dev)

    def model():
        torch.manual_seed(0)
        m = NeRFNetwork(bound=1, cuda_ray=True).to(dev)
        m.density_bitfield.copy_(bits)
        return m

    probe = FusedTrainer(model(), lego, M=args.num_rays * 64)
    counts = []
    for _ in range(4):
        probe.step()
        counts.append(probe.sample_count())
    M = int(np.mean(counts) * 1.25)
    del probe
    torch.cuda.empty_cache()

    trainers = {}
    for name, w in (("dist_off", 0.0), ("dist_on", args.weight)):
        ft = FusedTrainer(model(), lego, M=M, dist_loss_weight=w)
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
    over = {name: 0 for name in trainers}
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
            over[name] += int(ft.over_budget(16))

    # the composite launch itself: per-launch device times of the step body as the graphs run it
    body = {}
    for name, t in trainers.items():
        mean, _, cnt = t.timed_body_steps(args.body_steps)
        live = [k / max(n, 1) for k, n in zip(t.body_live_counts, cnt)] if t.body_live_counts else None
        body[name] = {"launch_ms": mean, "composite_loss_us": 1e3 * mean.get("composite_loss", float("nan")),
                      "mean_samples": float(np.mean(cnt)),
                      "live_row_share": float(np.mean(live)) if live else None}

    med = {name: float(np.median(v)) for name, v in ms.items()}
    on = trainers["dist_on"]
    result = {
        "config": {"H": lego.H, "W": lego.W, "n_poses": int(lego.poses.shape[0]), "num_rays": args.num_rays, "M": M,
                   "weight": args.weight, "steps": args.steps, "repeats": args.repeats,
                   "graph_steps": args.graph_steps, "device": torch.cuda.get_device_name(0)},
        "ms_per_step": ms,
        "median_ms_per_step": med,
        "spread_ms": {name: float(max(v) - min(v)) for name, v in ms.items()},
        "on_minus_off_ms": med["dist_on"] - med["dist_off"],
        "ratio_on_to_off": med["dist_on"] / med["dist_off"],
        "body_launches": body,
        "composite_on_minus_off_us": body["dist_on"]["composite_loss_us"] - body["dist_off"]["composite_loss_us"],
        "last_sample_counts": samples,
        "over_budget_steps": over,
        "losses": {name: t.last_loss for name, t in trainers.items()},
        "dist_term": on.last_dist_loss,
        "device_errors": {name: t.device_errors() for name, t in trainers.items()},
    }
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
