"""A/B of error-map importance sampling at Config 2 (800 x 800, 100 poses, 4096
rays, Lego occupancy), by the method of tools/image_source_ab.py: the image
source with a uint8 RGBA stack, its map off against on (128 x 128 cells), the
same model, seed and sample buffer. One build, one process: each trainer
captures its multi-step graph, both settle, then `--repeats` interleaved rounds
time `--steps` steps of each with device events. The select kernel's own time
is a graph of `--select-launches` back-to-back launches (res 128, N rays) on
the trained map, timed the same way. Writes a JSON.

    python tools/error_map_ab.py --out profiles/<tag>_error_map.json
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
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--select-launches", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import _ngp_native as nat
    from image_source_ab import ImageLego, render_stack
    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield

    dev = torch.device("cuda:0")
    lego = SyntheticLego(dev, num_rays=args.num_rays)
    u8 = render_stack(lego)
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
    # (the map concentrates the rays on the object, several times the uniform draw's
    # samples a step; rows past a step's count cost nothing)
    M = int(np.mean(counts) * 8)
    del probe
    torch.cuda.empty_cache()

    off, on = ImageLego(lego, u8), ImageLego(lego, u8)
    on.error_map = torch.ones(lego.poses.shape[0], args.res ** 2, device=dev)
    on.error_map_res = args.res
    trainers = {}
    for name, data in (("map_off", off), ("map_on", on)):
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

    # where the difference sits: per-launch device times of the step body as the graphs run it
    body = {}
    for name, t in trainers.items():
        mean, _, cnt = t.timed_body_steps(32)
        body[name] = {"launch_ms": mean, "mean_samples": float(np.mean(cnt))}

    # the select kernel alone: a graph of back-to-back launches on the trained map
    ft = trainers["map_on"]
    ft.flush()
    lib, P = nat.lib(), nat.ptr
    sel = torch.zeros(args.num_rays, dtype=torch.int32, device=dev)

    def launches():
        for _ in range(args.select_launches):
            nat.check(lib.ngp_error_map_select(P(on.error_map), lego.poses.shape[0], args.res, args.num_rays, 0,
                                               P(ft.state), P(sel), None, nat.stream_of(sel)), "select")
    launches()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launches()
    sel_us = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        sel_us.append(a.elapsed_time(b) * 1e3 / args.select_launches)

    med = {name: float(np.median(v)) for name, v in ms.items()}
    m = on.error_map
    result = {
        "config": {"H": lego.H, "W": lego.W, "n_poses": int(lego.poses.shape[0]), "num_rays": args.num_rays, "M": M,
                   "res": args.res, "steps": args.steps, "repeats": args.repeats, "graph_steps": args.graph_steps,
                   "device": torch.cuda.get_device_name(0)},
        "ms_per_step": ms,
        "median_ms_per_step": med,
        "spread_ms": {name: float(max(v) - min(v)) for name, v in ms.items()},
        "on_minus_off_ms": med["map_on"] - med["map_off"],
        "ratio_on_to_off": med["map_on"] / med["map_off"],
        "body_launches": body,
        "select_us_per_launch": sel_us,
        "select_us_median": float(np.median(sel_us)),
        "last_sample_counts": samples,
        "over_budget_steps": over,
        "losses": {name: t.last_loss for name, t in trainers.items()},
        "device_errors": {name: t.device_errors() for name, t in trainers.items()},
        "map": {"min": float(m.min()), "max": float(m.max()), "mean": float(m.mean()),
                "finite": bool(torch.isfinite(m).all())},
    }
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
