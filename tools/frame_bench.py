"""Per-frame time of a test render up to finished uint8 frames, two paths on one
trained field (the Lego bitfield, 800x800 unless --size), one process:

  (a) today's: get_rays + FusedRenderer.render as nerf.eval.psnr runs it, the
      float32 image and depth read back and quantised on the host with the
      reference's (x * 255).astype(np.uint8);
  (b) nerf.frames: FrameRenderer.frames() (ngp_frame_begin / _finish, the uint8
      frames read back through the pinned pair).

Each with and without PNG files: (a) saves the two files in line, as the
reference's loop does (nerf/utils.py:785-786); (b) is nerf.frames.write_frames
(4 encoder threads). The four variants are interleaved within every repeat;
the result holds each repeat's ms per frame, their median and range.

    python tools/frame_bench.py [--frames 20] [--repeats 7] [--out profiles/frame_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from nerf.frames import FrameRenderer, write_frames  # noqa: E402
from nerf.fused import FusedTrainer  # noqa: E402
from nerf.fused_render import FusedRenderer  # noqa: E402
from nerf.network_ff import NeRFNetwork  # noqa: E402
from nerf.provider import SyntheticLego, lego_bitfield  # noqa: E402
from nerf.utils import get_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "frame_bench.json"))
    a = ap.parse_args()
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
    model.eval()
    H = W = a.size
    poses = data.poses[torch.linspace(0, data.poses.shape[0] - 1, a.frames).long()]

    old = FusedRenderer(model, H * W)
    old.load_weights()
    old.capture()
    new = FrameRenderer(model, H, W, data.intrinsics)
    new.load_weights()
    new.capture()
    new.set_poses(poses)

    def old_frames():
        for i in range(a.frames):
            rays = get_rays(poses[i:i + 1], data.intrinsics, H, W, -1)
            out = old.render(rays["rays_o"], rays["rays_d"], bg_color=1)
            with np.errstate(invalid="ignore"):
                rgb = (out["image"].reshape(H, W, 3).cpu().numpy() * 255).astype(np.uint8)
                depth = (out["depth"].reshape(H, W).cpu().numpy() * 255).astype(np.uint8)
            yield rgb, depth

    def a_plain(_):
        for _f in old_frames():
            pass

    def b_plain(_):
        for _f in new.frames():
            pass

    def a_png(d):
        for i, (rgb, depth) in enumerate(old_frames()):
            Image.fromarray(rgb).save(os.path.join(d, f"a_{i:04d}_rgb.png"), compress_level=1)
            Image.fromarray(depth).save(os.path.join(d, f"a_{i:04d}_depth.png"), compress_level=1)

    def b_png(d):
        write_frames(new, d, "b")

    variants = {"a_float_readback_host_quantise": a_plain, "b_frame_kernels_uint8_readback": b_plain,
                "a_with_png_inline": a_png, "b_with_png_write_frames": b_png}
    # the two paths give the same pictures (rays_d differs in the last bits: DESIGN.md §14)
    same = [float((np.abs(x[0].astype(np.int32) - y[0].astype(np.int32)) <= 1).mean())
            for x, y in zip(old_frames(), ((r.copy(), d.copy()) for r, d in new.frames()))]
    times = {k: [] for k in variants}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(a.repeats + 1):  # repeat 0 warms every variant up
            for name, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(tmp)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(1e3 * (time.perf_counter() - t0) / a.frames)
    res = {"what": "ms per frame up to finished uint8 frames (and PNG files), host clock around synchronised work",
           "size": [H, W], "frames_per_repeat": a.frames, "repeats": a.repeats, "train_steps_before": a.train_steps,
           "device": torch.cuda.get_device_name(0),
           "colour_values_within_one_level_a_vs_b_min": round(min(same), 6),
           "ms_per_frame": {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                "max": round(max(v), 3), "repeats": [round(x, 3) for x in v]}
                            for k, v in times.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
