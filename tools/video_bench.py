"""The device JPEG encoder and the video path on one trained field (the Lego
bitfield, 800x800 unless --size), one process:

  encode   per frame of the path, device events around the three launches of
           ngp_jpeg_encode for the RGB frame and for the grey depth frame, and
           the scan's bytes (render and encode alternate, as in write_video);
  fps      write_video(png=False), write_video(png=True) and write_frames over
           the same path, interleaved within every repeat, host clock around
           synchronised work.

The times of the three launches one by one come from a kernel trace of
`--mode encode` (rocprofv3 --kernel-trace --output-format csv); --trace-csv folds
such a trace's k_jpeg_* rows into the result.

    python tools/video_bench.py [--frames 100] [--repeats 5] [--out profiles/video_bench.json]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd")]


def stats(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def fold_trace(path):
    """Per k_jpeg_* kernel of a rocprofv3 kernel-trace CSV: its durations in
    microseconds, the RGB image's launches and the grey image's apart (every
    frame encodes RGB first, then grey, so they alternate in start order)."""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in ("k_jpeg_transform", "k_jpeg_code", "k_jpeg_compact"):
                if k in row.get("Kernel_Name", ""):
                    start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                    rows.setdefault(k, []).append((start, (end - start) / 1e3, row))
    res = {}
    for k, v in rows.items():
        v.sort(key=lambda r: r[0])
        v = v[len(v) // 2:]  # the second pass over the path (the first warms up)
        res[k] = {label + "_us": dict(stats([us for _, us, _ in v[first::2]]), launches=len(v[first::2]))
                  for label, first in (("rgb", 0), ("grey", 1))}
        for key in ("VGPR_Count", "Accum_VGPR_Count", "SGPR_Count", "LDS_Block_Size", "Scratch_Size",
                    "Workgroup_Size_X", "Grid_Size_X", "Workgroup_Size", "Grid_Size"):
            if key in v[0][2]:
                res[k][key.lower()] = int(v[0][2][key])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["all", "encode", "fold"], default="all",
                    help="fold: only put --trace-csv's launches into the existing --out file (no GPU)")
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--trace-csv", type=str, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "video_bench.json"))
    a = ap.parse_args()
    if a.mode == "fold":
        with open(a.out) as f:
            res = json.load(f)
        res["launches_from_kernel_trace"] = fold_trace(a.trace_csv)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["launches_from_kernel_trace"]))
        return

    import torch

    from nerf.frames import FrameRenderer, write_frames, write_video
    from nerf.fused import FusedTrainer
    from nerf.jpeg import JpegEncoder
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield

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
    fr = FrameRenderer(model, H, W, data.intrinsics)
    fr.load_weights()
    fr.capture()
    fr.set_poses(poses)

    encoders = {"rgb": JpegEncoder(H, W, 3, a.quality, dev), "grey": JpegEncoder(H, W, 1, a.quality, dev)}
    ms = {k: [] for k in encoders}
    size = {k: [] for k in encoders}
    events = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(a.frames)] for k in encoders}
    render_ms = []
    for rep in range(2):  # pass 0 warms up
        for i in range(a.frames):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            rgb8, depth8 = fr.render(i)
            t1.record()
            for k, image in (("rgb", rgb8), ("grey", depth8)):
                events[k][i][0].record()
                encoders[k].launch(image)
                events[k][i][1].record()
            torch.cuda.synchronize()
            if rep:
                render_ms.append(t0.elapsed_time(t1))
                for k in encoders:
                    ms[k].append(events[k][i][0].elapsed_time(events[k][i][1]))
                    size[k].append(int(encoders[k].scan_len.item()))
    res = {"what": "device JPEG encoder (quality %d) and the video path; encode: device events around the three "
                   "launches of one image, ms; fps: ms per frame, host clock around synchronised work" % a.quality,
           "size": [H, W], "frames": a.frames, "train_steps_before": a.train_steps,
           "device": torch.cuda.get_device_name(0),
           "render_ms_device_events": stats(render_ms),
           "encode_ms": {k: stats(v, 4) for k, v in ms.items()},
           "scan_bytes": {k: dict(stats(v, 0), bytes_per_pixel=round(statistics.mean(v) / (H * W), 4),
                                  capacity=encoders[k].capacity) for k, v in size.items()}}
    if a.trace_csv:
        res["launches_from_kernel_trace"] = fold_trace(a.trace_csv)

    if a.mode == "all":
        def video_only(d):
            write_video(fr, d, "v", quality=a.quality, png=False)

        def video_png(d):
            write_video(fr, d, "w", quality=a.quality, png=True)

        def png_only(d):
            write_frames(fr, d, "p")

        variants = {"write_video_png_false": video_only, "write_video_png_true": video_png,
                    "write_frames": png_only}
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
            res["avi_bytes"] = {k: os.path.getsize(os.path.join(tmp, f"v_{k}.avi")) for k in ("rgb", "depth")}
        res["repeats"] = a.repeats
        res["ms_per_frame"] = {k: dict(stats(v), repeats=[round(x, 3) for x in v],
                                       frames_per_second=round(1e3 / statistics.median(v), 1))
                               for k, v in times.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
