"""Times what mesh export does after marching cubes (csrc/mesh_clean.hip,
nerf/mesh.py components / clean / vertex_colors) on the GPU, per stage, on
mesh_bench.py's set-up: the three-box model trained with the fused engine,
meshed at --resolution. Beside them the same run's (a)-(d)
rows of §11, measured as mesh_bench.py measures them.

  labelling        ngp_mesh_components: init, hook, compress + count
  clean count      ngp_mesh_clean_count: roots, flags, sums, scan, prefix
  clean emit       ngp_mesh_clean_emit (the rule: --min_faces, largest only)
  colours          vertex_colors for all V vertices of the raw mesh
  host read        the 32-byte read of the clean's counts
  save_mesh        end to end, plain and with all three options
  scipy (context)  scipy.sparse.csgraph.connected_components on the same
                   faces on the host, the copy of the faces not included

Every figure is the median of `--repeats` timed runs after `--warmup` untimed
ones, with min and max: device events around `--inner` back-to-back calls for
the kernels, the host clock around a device synchronise for the rest. No GPU:
an error, never a CPU figure.

usage: python tools/mesh_clean_bench.py [--steps 1000] [--resolution 256] [--min_faces 50] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd"), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mesh_bench import events, stats, train, wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=10.0)
    ap.add_argument("--min_faces", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_bench: no GPU (a CPU run measures nothing)")
    import _ngp_native as nat
    from nerf import mesh
    dev = torch.device("cuda:0")
    lib, P = nat.lib(), nat.ptr
    R, thr, W, K, I = args.resolution, args.threshold, args.warmup, args.repeats, args.inner
    t0 = time.perf_counter()
    model, ft = train(dev, args.steps)
    res = {"resolution": R, "threshold": thr, "train_steps": args.steps,
           "train_seconds": round(time.perf_counter() - t0, 2), "loss": ft.last_loss,
           "device": torch.cuda.get_device_name(0), "min_faces": args.min_faces,
           "method": f"median of {K} runs after {W} warm-up; kernels: device events around {I} calls; the rest: "
                     f"host clock around a synchronise"}

    # the §11 rows of this run
    res["a_sample_density"] = wall(lambda: mesh.sample_density(model, R), W, K)
    vol = mesh.sample_density(model, R)
    box = mesh._aabb_list(model.aabb_infer)
    res["bcd_marching_cubes_with_read"] = wall(lambda: mesh.marching_cubes(vol, thr, aabb=box, normals=True), W, K)
    verts, faces, nrm = mesh.marching_cubes(vol, thr, aabb=box, normals=True)
    V, T = int(verts.shape[0]), int(faces.shape[0])
    res.update(vertices=V, triangles=T)
    s = nat.stream_of(verts)

    # the labelling
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    comp_faces = torch.empty(V, dtype=torch.int32, device=dev)

    def label():
        nat.check(lib.ngp_mesh_components(P(faces), V, T, P(labels), P(comp_faces), s), "mesh_components")
    res["labelling"] = events(label, W, K, I)

    # the clean
    ws_bytes = int(lib.ngp_mesh_clean_workspace_bytes(V, T))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    res["clean_workspace_bytes"] = ws_bytes
    for name, mf, kl in (("min_faces", args.min_faces, 0), ("all_flags", args.min_faces, 1)):
        def count():
            nat.check(lib.ngp_mesh_clean_count(P(faces), V, T, P(labels), P(comp_faces), mf, kl, P(ws), ws_bytes,
                                               P(counts), s), "mesh_clean_count")
        res[f"clean_count_{name}"] = events(count, W, K, I)
        V2, T2, ncomp, nkept = (int(c) for c in counts.cpu().tolist())
        res[f"result_{name}"] = dict(vertices=V2, triangles=T2, components=ncomp, components_kept=nkept)
        v2, n2 = torch.empty(max(V2, 1), 3, device=dev), torch.empty(max(V2, 1), 3, device=dev)
        f2 = torch.empty(max(T2, 1), 3, dtype=torch.int32, device=dev)

        def emit():
            nat.check(lib.ngp_mesh_clean_emit(P(verts), P(nrm), P(faces), V, T, P(ws), ws_bytes, V2, T2, P(v2), P(n2),
                                              P(f2), s), "mesh_clean_emit")
        res[f"clean_emit_{name}"] = events(emit, W, K, I)
    res["clean_counts_host_read"] = wall(lambda: counts.cpu(), W, K)
    res["clean_python"] = wall(lambda: mesh.clean(verts, faces, nrm, min_faces=args.min_faces, keep_largest=True),
                               W, K)

    # the colours
    res["vertex_colors_all"] = wall(lambda: mesh.vertex_colors(model, verts, nrm), W, K)
    res["vertices_per_second_colors"] = round(V / (res["vertex_colors_all"]["median_ms"] * 1e-3)) if V else 0

    # end to end
    with tempfile.TemporaryDirectory(prefix="mesh_clean_bench_") as tmp:
        ply = os.path.join(tmp, "bench.ply")
        res["save_mesh_plain"] = wall(lambda: mesh.save_mesh(model, ply, R, thr), 1, 3)
        res["ply_bytes_plain"] = os.path.getsize(ply)
        res["save_mesh_all_flags"] = wall(lambda: mesh.save_mesh(model, ply, R, thr, colors=True,
                                                                 min_faces=args.min_faces, keep_largest=True), 1, 3)
        res["ply_bytes_all_flags"] = os.path.getsize(ply)

    # context: the host library on the same faces
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        res["scipy_connected_components"] = None
    else:
        f = faces.cpu().numpy().astype(np.int64)

        def host():
            e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]]])
            g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(V, V))
            return connected_components(g, directed=False)
        out = []
        for i in range(1 + 3):
            t = time.perf_counter()
            n_host, _ = host()
            if i:
                out.append((time.perf_counter() - t) * 1e3)
        res["scipy_connected_components"] = stats(out)
        res["scipy_components"] = int(n_host)
    res["device_errors"] = ft.device_errors()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
