"""Times one SDF training step (sdf/, csrc/sdf.hip) on the GPU, split into its
parts, on a procedurally built torus at about 100k triangles and at 1,024
(DESIGN.md §21):

  sample          ngp_sdf_sample, N points
  query plain     ngp_sdf_query on the batch's second half, every face scanned
  query culled    the same with the block cull, the points in the batch's order
  query sorted    the cull on Morton-sorted points: the sort, the gathers and
                  the scatter included (what SDFDataset(sort=True) enqueues),
                  and the kernel alone on points sorted beforehand
  network         forward, mape, backward and the fused Adam on a fixed batch
  step            SDFTrainer.train_step end to end with the default dataset

Every figure is the median of `--repeats` rounds after `--warmup` untimed
ones, with min and max; a round times every variant once, one after the other
(interleaved), with device events around `--inner` back-to-back calls. The
culled and the plain results are compared bit for bit on the way. --yardstick
adds the training test's figures (tests/test_gpu_sdf.py): the plain torch
trainer's and the device trainer's error over three seeds. No GPU: an error,
never a CPU figure.

usage: python tools/sdf_bench.py [--num_samples 262144] [--out profiles/sdf_bench.json] [--yardstick]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd"), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def torus(nu, nv, R=1.0, r=0.4):
    u, w = 2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv
    U, W = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v, f


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def interleaved(variants, warmup, repeats, inner):
    """variants: name -> callable. One round runs every variant once."""
    times = {k: [] for k in variants}
    for r in range(warmup + repeats):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b) / inner)
    return {k: stats(v) for k, v in times.items()}


def bench_mesh(dev, nu, nv, N, args):
    import sdf
    from sdf.provider import morton_perm, new_counter, sdf_query, sdf_sample
    mesh = sdf.prepare_mesh(*torus(nu, nv), device=dev)
    counter = new_counter(dev)
    points, tri = sdf_sample(mesh, N, 0, counter)
    h = N // 2
    pts, t = points[h:].contiguous(), tri[h:].contiguous()
    out = torch.empty(h, device=dev)
    perm = morton_perm(pts, t < 0)
    spts, st = pts[perm].contiguous(), t[perm].contiguous()

    def sorted_path():
        p = morton_perm(pts, t < 0)
        out[p] = sdf_query(mesh, pts[p].contiguous(), t[p].contiguous(), cull=True)

    plain = sdf_query(mesh, pts, t, cull=False, feature=True)
    culled = sdf_query(mesh, pts, t, cull=True, feature=True)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, culled))
    sorted_path()
    same_sorted = torch.equal(out.abs().view(torch.int32), plain[0].abs().view(torch.int32))

    model = sdf.SDFNetwork().to(dev)
    fixed = sdf.SDFDataset(mesh, num_samples=N, seed=0)
    trainer = sdf.SDFTrainer(model, fixed)
    batch = {k: v.clone() for k, v in fixed.sample().items()}

    def network():
        model.train()
        trainer.optimizer.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            pred = model(batch["points"])
        loss = sdf.mape_loss(pred, batch["sdfs"])
        trainer.scaler.scale(loss).backward()
        trainer.scaler.step(trainer.optimizer)
        trainer.scaler.update()

    variants = {
        "sample": lambda: sdf_sample(mesh, N, 0, counter, points, tri),
        "query_plain": lambda: sdf_query(mesh, pts, t, cull=False, out=out),
        "query_culled": lambda: sdf_query(mesh, pts, t, cull=True, out=out),
        "query_sorted_with_sort": sorted_path,
        "query_sorted_kernel_only": lambda: sdf_query(mesh, spts, st, cull=True, out=out),
        "network_fwd_bwd_adam": network,
        "step": trainer.train_step,
    }
    res = interleaved(variants, args.warmup, args.repeats, args.inner)
    res.update(triangles=mesh.T, blocks=int(mesh.block_aabb.shape[0]), num_samples=N, query_points=h,
               culled_equals_plain_bits=bool(same), sorted_equals_plain_distance_bits=bool(same_sorted),
               dataset_sorts_points=bool(fixed.sort))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_samples", type=int, default=2 ** 18)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdf_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"median of {args.repeats} interleaved rounds after {args.warmup} warm-up rounds; device events "
                     f"around {args.inner} back-to-back calls"}
    res["torus_100k"] = bench_mesh(dev, 320, 157, args.num_samples, args)
    res["torus_1024"] = bench_mesh(dev, 32, 16, args.num_samples, args)
    if args.yardstick:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_gpu_sdf as t
        m = t.mesh_of("torus_96", dev)
        yard = [t.yardstick_error(m, dev, seed=s) for s in range(3)]
        device = [t.device_error(m, dev, seed=s)[0] for s in range(3)]
        res["training_yardstick"] = {
            "steps": t.TRAIN_STEPS, "num_samples": t.TRAIN_N, "mesh": "torus_96",
            "yardstick_error_seeds_0_1_2": yard, "device_error_seeds_0_1_2": device,
            "yardstick_spread_max_over_min": max(yard) / min(yard), "allowed_ratio": t.YARDSTICK_RATIO}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
