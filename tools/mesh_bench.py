"""Times the mesh export (nerf/mesh.py, csrc/mesh.hip) on the GPU, per stage,
on a three-box model trained with the fused engine.

  (a) sampling        sample_density: lattice points + fused grid forward +
                      sigma network, chunked
  (b) count + scans   ngp_mesh_count (k_mesh_count, k_mesh_scan_blocks,
                      k_mesh_prefix)
  (c) emit            ngp_mesh_emit, without and with normals
  (d) host            the 16-byte read of the counts; the outputs' copy to the
                      host and the PLY write
  (e) reference shape model.density() under autocast over the same lattice in
                      128^3 chunks, each copied to the host into a numpy volume
                      (the reference's extract_fields, nerf/utils.py:172-187;
                      its marching-cubes step needs PyMCubes and is not timed)

Every figure is the median of `--repeats` timed runs after `--warmup` untimed
ones, with min and max; (a), (d), (e) on the host clock around a device
synchronise, (b), (c) with device events around `--inner` back-to-back calls
(a single call is too short for the clock). Bytes are what the passes must
move, from the shapes (bytes_model below), over the measured time. No GPU: an
error, never a CPU figure.

usage: python tools/mesh_bench.py [--steps 1000] [--resolution 256] [--threshold 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "runs": len(ms)}


def wall(fn, warmup, repeats):
    out = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return stats(out)


def events(fn, warmup, repeats, inner):
    out = []
    for i in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b) / inner)
    return stats(out)


def train(dev, steps, every=16):
    """main_nerf's loop on the three-box scene."""
    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    model.train()
    data = SyntheticLego(dev, num_rays=4096)
    model.mark_untrained_grid(data.poses, data.intrinsics)
    ft = FusedTrainer(model, data, M=2 ** 20, seed=0)
    done, captured = 0, False
    while done < steps:
        ft.update_density()
        k = min(every, steps - done)
        if captured:
            ft.run(k)
        else:
            for _ in range(k):
                ft.step()
            if k == every and done + k < steps:
                ft.capture(warmup=0, multi=max(every - 1, 1))
                captured = True
        done += k
    ft.flush()
    torch.cuda.synchronize()
    return model, ft


def bytes_model(N, V, T, normals):
    """What the passes must move, from the shapes."""
    count = {"volume_read": 4 * N, "flags_tricount_written": 2 * N}
    prefix = {"flags_tricount_read": 2 * N, "prefixes_written": 8 * N}
    emit = {"volume_read": 4 * N, "flags_read": N, "prefixes_read": 8 * N,
            "vertices_written": 12 * V * (2 if normals else 1), "faces_written": 12 * T}
    return {"count": count, "prefix": prefix, "emit": emit,
            "count_total": sum(count.values()) + sum(prefix.values()), "emit_total": sum(emit.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench: no GPU (a CPU run measures nothing)")
    import _ngp_native as nat
    from nerf import mesh
    dev = torch.device("cuda:0")
    lib, P = nat.lib(), nat.ptr
    R, thr = args.resolution, args.threshold
    N = R ** 3
    t0 = time.perf_counter()
    model, ft = train(dev, args.steps)
    train_s = time.perf_counter() - t0
    res = {"resolution": R, "threshold": thr, "train_steps": args.steps, "train_seconds": round(train_s, 2),
           "loss": ft.last_loss, "device": torch.cuda.get_device_name(0),
           "method": f"median of {args.repeats} runs after {args.warmup} warm-up; (a)(d)(e) host clock around a "
                     f"synchronise, (b)(c) device events around {args.inner} calls"}

    # (a) sampling
    res["a_sample_density"] = wall(lambda: mesh.sample_density(model, R), args.warmup, args.repeats)
    vol = mesh.sample_density(model, R)
    res["sigma_max"] = float(vol.max())
    res["points_per_second_a"] = round(N / (res["a_sample_density"]["median_ms"] * 1e-3))

    # (b) count + scans
    ws_bytes = int(lib.ngp_mesh_workspace_bytes(R, R, R))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    s = nat.stream_of(vol)

    def count():
        nat.check(lib.ngp_mesh_count(P(vol), R, R, R, thr, P(ws), ws_bytes, P(counts), s), "mesh_count")
    res["b_count_scans"] = events(count, args.warmup, args.repeats, args.inner)
    res["d_counts_host_read"] = wall(lambda: counts.cpu(), args.warmup, args.repeats)
    V, T = (int(c) for c in counts.cpu().tolist())
    res.update(vertices=V, triangles=T, workspace_bytes=ws_bytes)

    # (c) emit
    box = mesh._aabb6(model.aabb_infer)
    verts = torch.empty(max(V, 1), 3, device=dev)
    nrm = torch.empty(max(V, 1), 3, device=dev)
    faces = torch.empty(max(T, 1), 3, dtype=torch.int32, device=dev)
    if V or T:
        for name, n in (("c_emit", None), ("c_emit_normals", nrm)):
            def emit():
                nat.check(lib.ngp_mesh_emit(P(vol), R, R, R, thr, box, P(ws), ws_bytes, V, T, P(verts), P(n),
                                            P(faces), s), "mesh_emit")
            res[name] = events(emit, args.warmup, args.repeats, args.inner)
            bm = bytes_model(N, V, T, n is not None)
            t_bc = (res["b_count_scans"]["median_ms"] + res[name]["median_ms"]) * 1e-3
            res[name + "_bytes"] = bm
            res[name + "_bc_GBps"] = round((bm["count_total"] + bm["emit_total"]) / t_bc / 1e9, 1)
        res["b_GBps"] = round(bytes_model(N, V, T, False)["count_total"]
                              / (res["b_count_scans"]["median_ms"] * 1e-3) / 1e9, 1)

    # (d) the outputs to the host and the PLY write
    with tempfile.TemporaryDirectory(prefix="mesh_bench_") as tmp:
        ply = os.path.join(tmp, "bench.ply")

        def write():
            mesh.write_ply(ply, verts[:V].cpu().numpy(), faces[:T].cpu().numpy(), nrm[:V].cpu().numpy())
        res["d_copy_and_ply_write"] = wall(write, 1, max(3, args.repeats // 3))
        res["ply_bytes"] = os.path.getsize(ply)
        # the whole export as a user calls it
        res["save_mesh_total"] = wall(lambda: mesh.save_mesh(model, ply, R, thr), 1, 3)

    # (e) the reference-shaped sampling: density() in 128^3 chunks, each to the host
    def reference_shape():
        aabb = model.aabb_infer
        axes = [torch.linspace(float(aabb[a]), float(aabb[a + 3]), R, device=dev).split(128) for a in range(3)]
        u = np.zeros([R, R, R], dtype=np.float32)
        with torch.no_grad():
            for xi, xs in enumerate(axes[0]):
                for yi, ys in enumerate(axes[1]):
                    for zi, zs in enumerate(axes[2]):
                        xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                        pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                        with torch.autocast("cuda", dtype=torch.float16):
                            sigma = model.density(pts)["sigma"]
                        val = sigma.reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
                        u[xi * 128: xi * 128 + len(xs), yi * 128: yi * 128 + len(ys),
                          zi * 128: zi * 128 + len(zs)] = val
        return u
    res["e_reference_shaped_sampling"] = wall(reference_shape, 1, max(3, args.repeats // 3))
    res["a_over_e"] = round(res["a_sample_density"]["median_ms"] / res["e_reference_shaped_sampling"]["median_ms"], 4)
    if "c_emit" in res:
        res["bc_over_a"] = round((res["b_count_scans"]["median_ms"] + res["c_emit_normals"]["median_ms"])
                                 / res["a_sample_density"]["median_ms"], 4)
    res["device_errors"] = ft.device_errors()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
