"""What SSIM adds to the validation pass, on the partly
trained Lego field of tools/validate_bench.py (800x800 views unless --size), one
process, the variants interleaved within every repeat:

  (a) Validator.run() with ssim=False, ms per view: today's pass. The tool also
      runs on a tree without SSIM (it then measures (a) alone), so the same
      number can be taken on the parent commit;
  (b) Validator.run() with ssim=True, ms per view, and its difference to (a) in
      the same repeat; beside it the device-event time of ngp_frame_ssim alone
      over back-to-back calls on one rendered view (and of ngp_frame_sse, for
      scale);
  (c) the obvious alternative on the device: the float image and a float
      ground truth through torch.nn.functional.conv2d in float64 (the five
      moments as 15 planes, a 1 x 11 and an 11 x 1 pass, the formula, the mean),
      device-event ms per view, and how far its mean is from the kernel's.

    python tools/ssim_bench.py [--views 10] [--repeats 7] [--out profiles/ssim_bench.json]
"""
import argparse
import ctypes
import inspect
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
from nerf.eval import Validator, ground_truth  # noqa: E402
from nerf.fused import FusedTrainer  # noqa: E402
from nerf.network_ff import NeRFNetwork  # noqa: E402
from nerf.provider import SyntheticLego, lego_bitfield  # noqa: E402
from nerf.utils import get_rays  # noqa: E402


def _summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "repeats": [round(x, 4) for x in v]}


def _events(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernel-calls", type=int, default=50, help="back-to-back metric launches per timed window")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ssim_bench.json"))
    a = ap.parse_args()
    has_ssim = "ssim" in inspect.signature(Validator.__init__).parameters
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True).to(dev)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield()).to(dev))
    data = SyntheticLego(dev, H=a.size, W=a.size, num_rays=4096)
    ft = FusedTrainer(model, data, M=101762)
    for _ in range(a.train_steps):  # a partly trained field, so rays terminate as in a test render
        ft.step()
    ft.flush()
    torch.cuda.synchronize()
    H = W = a.size
    idx = torch.linspace(0, data.poses.shape[0] - 1, a.views).long()
    images = []
    for k in idx.tolist():
        rays = get_rays(data.poses[k:k + 1], data.intrinsics, H, W, -1)
        images.append((data.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4) * 255).round().to(torch.uint8))
    val = types.SimpleNamespace(poses=data.poses[idx].contiguous(), intrinsics=data.intrinsics, H=H, W=W,
                                images=torch.stack(images).contiguous(), depths=None)
    model.eval()

    plain = Validator(model, val)
    variants = {"a_validator_run": plain.run}
    if has_ssim:
        with_ssim = Validator(model, val, ssim=True)
        variants["b_validator_run_ssim"] = with_ssim.run
    times, last = {k: [] for k in variants}, {}
    for rep in range(a.repeats + 1):  # repeat 0 warms every variant up (and captures the graphs)
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(1e3 * (time.perf_counter() - t0) / a.views)
    res = {"what": "validation: ms per view, host clock around synchronised passes of all views; kernels and the "
                   "conv2d alternative: device events",
           "device": torch.cuda.get_device_name(0), "size": [H, W], "views": a.views, "repeats": a.repeats,
           "train_steps_before": a.train_steps, "tree_has_ssim": has_ssim,
           "validation_ms_per_view": {k: _summary(v) for k, v in times.items()},
           "mean_psnr": last["a_validator_run"]["mean_psnr"]}
    if has_ssim:
        added = [b - x for x, b in zip(times["a_validator_run"], times["b_validator_run_ssim"])]
        res["b_added_ms_per_view"] = _summary(added)
        res["mean_ssim"] = last["b_validator_run_ssim"]["mean_ssim"]
        assert last["a_validator_run"]["mse"].tobytes() == last["b_validator_run_ssim"]["mse"].tobytes()

        # the metric launches alone, on the last view's render
        v, P = with_ssim, nat.ptr
        r = v.frames.renderer
        view = a.views - 1
        v.frames.render(view, floats=True)  # (leaves r.image and r.weights_sum of this view)
        bg = 0.0 if r._bg else v.frames.bg_color

        def k_ssim():
            nat.check(nat.lib().ngp_frame_ssim(H, W, P(r.image), P(r.weights_sum), bg, ctypes.byref(v._src), view,
                                               P(v.ssim), None, r._stream()), "frame_ssim")

        def k_sse():
            nat.check(nat.lib().ngp_frame_sse(H, W, P(r.image), P(r.weights_sum), bg, ctypes.byref(v._src), view,
                                              P(v.sse), r._stream()), "frame_sse")

        # (c) float64 conv2d on the float image and a float ground truth
        g = torch.from_numpy(np.exp(-(np.arange(11) - 5.0) ** 2 / (2 * 1.5 ** 2))).to(dev)
        g = g / g.sum()
        wh, wv = g.reshape(1, 1, 1, 11).repeat(15, 1, 1, 1), g.reshape(1, 1, 11, 1).repeat(15, 1, 1, 1)
        gt = ground_truth(val, view).reshape(H, W, 3)
        C1, C2 = 0.01 * 0.01, 0.03 * 0.03
        conv_out = torch.zeros(1, dtype=torch.float64, device=dev)

        def c_conv2d():
            x = (r.image + (1 - r.weights_sum)[:, None] * bg).reshape(H, W, 3).permute(2, 0, 1).double()
            y = gt.permute(2, 0, 1).double()
            planes = torch.cat([x, y, x * x, y * y, x * y])[None]  # [1, 15, H, W]
            m = torch.nn.functional.conv2d(torch.nn.functional.conv2d(planes, wh, groups=15), wv, groups=15)[0]
            mux, muy = m[0:3], m[3:6]
            sx, sy, sxy = m[6:9] - mux * mux, m[9:12] - muy * muy, m[12:15] - mux * muy
            s = ((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sx + sy + C2))
            conv_out.copy_(s.mean().reshape(1))

        kernels = {"ngp_frame_ssim": k_ssim, "ngp_frame_sse": k_sse}
        try:
            c_conv2d()
            torch.cuda.synchronize()
            kernels["c_torch_conv2d_float64"] = c_conv2d
        except RuntimeError as e:  # no float64 convolution in this build
            res["c_torch_conv2d_float64_error"] = str(e).splitlines()[0]
        ms = {k: [] for k in kernels}
        for rep in range(a.repeats + 1):
            for name, fn in kernels.items():
                t = _events(fn, a.kernel_calls if name.startswith("ngp_") else 3)
                if rep:
                    ms[name].append(t)
        res["device_ms_per_view"] = {k: _summary(x) for k, x in ms.items()}
        torch.cuda.synchronize()
        mean_kernel = float(v.ssim[view]) / (3 * (H - 10) * (W - 10))
        res["ssim_of_last_view"] = {"ngp_frame_ssim": mean_kernel}
        if "c_torch_conv2d_float64" in kernels:
            res["ssim_of_last_view"]["conv2d_float64"] = float(conv_out[0])
            res["ssim_of_last_view"]["abs_difference"] = abs(float(conv_out[0]) - mean_kernel)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
