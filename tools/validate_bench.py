"""The validation pass and the EMA update against what they replace, on one
partly trained Lego field (800x800 views unless --size), one process:

  validation, ms per view over the same model and views:
    (a) nerf.eval.psnr per view with one shared FusedRenderer, as main_nerf's
        final evaluation runs it (get_rays in torch, render, blend, torch's
        float32 mean, .item()); that renderer is not captured, so its loop
        issues its launches eagerly;
    (a2) the same with the renderer's loop captured, the graph (b) replays: the
        difference to (a) is the eager launches, the difference to (b) is what
        the frame kernels and the device-side sum replace;
    (b) nerf.eval.Validator.run (ngp_frame_begin, the loop, ngp_frame_sse, one
        read-back per pass).
    The host synchronisations per view of each are counted: the render loop's
    state reads (one per graph replay or eager round), plus psnr's .item().

  EMA, one update at the trainer's flat parameter count:
    (c) ngp_ema_update over the flat buffer;
    (d) torch_ema's three operations per parameter tensor
        (tmp = s - p; tmp.mul_(1 - decay); s.sub_(tmp)).
    Device-event time per update; (c)'s bytes are the 12 per parameter it has
    to move (read s, read p, write s). Back to back the two buffers stay in the
    256 MB last-level cache, so each is also timed alone after a 1 GiB fill has
    evicted them, which is how the once-per-epoch update meets them.

The variants of each pair are interleaved within every repeat.

    python tools/validate_bench.py [--views 20] [--repeats 7] [--out profiles/validate_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _ngp_native as nat  # noqa: E402
from nerf.eval import Validator, psnr  # noqa: E402
from nerf.fused import FusedTrainer  # noqa: E402
from nerf.fused_render import FusedRenderer  # noqa: E402
from nerf.network_ff import NeRFNetwork  # noqa: E402
from nerf.provider import SyntheticLego, lego_bitfield  # noqa: E402
from nerf.utils import get_rays  # noqa: E402


def _summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "repeats": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ema-calls", type=int, default=50, help="EMA updates per timed window")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "validate_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True).to(dev)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield()).to(dev))
    data = SyntheticLego(dev, H=a.size, W=a.size, num_rays=4096)
    ft = FusedTrainer(model, data, M=101762, ema_decay=0.95)
    for _ in range(a.train_steps):  # a partly trained field, so rays terminate as in a test render
        ft.step()
    ft.flush()
    torch.cuda.synchronize()
    H = W = a.size
    # the views: the analytic target of `views` poses as the uint8 RGBA stack a scene's PNGs load to
    idx = torch.linspace(0, data.poses.shape[0] - 1, a.views).long()
    images = []
    for k in idx.tolist():
        rays = get_rays(data.poses[k:k + 1], data.intrinsics, H, W, -1)
        images.append((data.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4) * 255).round().to(torch.uint8))
    val = types.SimpleNamespace(poses=data.poses[idx].contiguous(), intrinsics=data.intrinsics, H=H, W=W,
                                images=torch.stack(images).contiguous(), depths=None)
    model.eval()

    old = FusedRenderer(model, H * W)
    old.load_weights()
    old_graph = FusedRenderer(model, H * W)
    old_graph.load_weights()
    old_graph.capture()
    new = Validator(model, val)
    reads = {"a": 0, "a2": 0, "b": 0}

    def psnr_pass(renderer, key):
        reads[key] = 0
        scores = []
        for i in range(a.views):
            scores.append(psnr(model, val, i, renderer=renderer))
            reads[key] += renderer.iterations // renderer.K + 1  # the loop's state reads, and .item()
        return scores

    def a_psnr():
        return psnr_pass(old, "a")

    def a2_psnr():
        return psnr_pass(old_graph, "a2")

    def b_validator():
        res = new.run()
        return list(res["psnr"])

    def b_reads():  # one more pass, counting the loop's state reads per view
        n = 0
        new.frames.load_weights()
        for i in range(a.views):
            new.sse_view(i)
            n += new.frames.renderer.iterations // new.frames.renderer.K
        return n

    variants = {"a_eval_psnr_per_view": a_psnr, "a2_eval_psnr_captured_loop": a2_psnr,
                "b_validator_run": b_validator}
    times, scores = {k: [] for k in variants}, {}
    for rep in range(a.repeats + 1):  # repeat 0 warms every variant up (and captures the validator's graph)
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scores[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(1e3 * (time.perf_counter() - t0) / a.views)
    reads["b"] = b_reads()
    diff = max(abs(x - y) for x, y in zip(scores["a_eval_psnr_per_view"], scores["b_validator_run"]))

    # the EMA update
    n = int(ft.total)
    shadows, params = ft.ema_params(), [p.detach() for p in ft.params]
    omd = float(np.float32(0.05))

    def c_kernel():
        nat.check(nat.lib().ngp_ema_update(nat.ptr(ft.ema_shadow), nat.ptr(ft.flat_param), n, omd,
                                           nat.stream_of(ft.flat_param)), "ema_update")

    def d_torch():
        for s, p in zip(shadows, params):
            tmp = s - p
            tmp.mul_(omd)
            s.sub_(tmp)

    ema_variants = {"c_ngp_ema_update": c_kernel, "d_torch_three_operations": d_torch}
    ema_ms = {k: [] for k in ema_variants}
    for rep in range(a.repeats + 1):
        for name, fn in ema_variants.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(a.ema_calls):
                fn()
            end.record()
            end.synchronize()
            if rep:
                ema_ms[name].append(start.elapsed_time(end) / a.ema_calls)
    # ... and one update at a time after a fill larger than the last-level cache
    evict = torch.empty(2 ** 30, dtype=torch.uint8, device=dev)
    cold_ms = {k: [] for k in ema_variants}
    for rep in range(a.repeats + 1):
        for name, fn in ema_variants.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            evict.fill_(rep & 255)
            start.record()
            fn()
            end.record()
            end.synchronize()
            if rep:
                cold_ms[name].append(start.elapsed_time(end))
    med_c = statistics.median(ema_ms["c_ngp_ema_update"])
    med_cold = statistics.median(cold_ms["c_ngp_ema_update"])
    res = {"what": "validation: ms per view, host clock around synchronised passes; EMA: ms per update, device events "
                   f"around {a.ema_calls} back-to-back updates",
           "device": torch.cuda.get_device_name(0), "size": [H, W], "views": a.views, "repeats": a.repeats,
           "train_steps_before": a.train_steps,
           "validation_ms_per_view": {k: _summary(v) for k, v in times.items()},
           "host_syncs_per_view": {"a_eval_psnr_per_view": round(reads["a"] / a.views, 2),
                                   "a2_eval_psnr_captured_loop": round(reads["a2"] / a.views, 2),
                                   "b_validator_run": round(reads["b"] / a.views, 2),
                                   "note": "a, a2: the loop's state reads + psnr's .item(); b: the loop's state reads "
                                           "(+ one read-back per pass)"},
           "psnr_max_abs_difference_a_vs_b": diff,
           "mean_psnr": {k: float(np.mean(v)) for k, v in scores.items()},
           "ema": {"parameters": n, "ms_per_update": {k: _summary(v) for k, v in ema_ms.items()},
                   "c_bytes_moved": 12 * n, "c_bytes_per_parameter_needed": 12,
                   "c_achieved_GB_per_s": round(12 * n / (med_c * 1e-3) / 1e9, 1),
                   "ms_per_update_after_cache_eviction": {k: _summary(v) for k, v in cold_ms.items()},
                   "c_achieved_GB_per_s_after_cache_eviction": round(12 * n / (med_cold * 1e-3) / 1e9, 1),
                   "d_bytes_per_parameter": 32}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
