"""Times TensoRF's vector-matrix sampling on the GPU: the kernel path
(tensoRF.vm_sample, csrc/tensorf.hip) against the torch path (vm_reference: 12
grid_sample calls on reference-layout tensors), forward + backward, on the
same inputs in the same process:

  sum16      the density set (ranks 16 16 16), `sum` mode
  concat48   the colour set (ranks 48 48 48), `concat` mode
  both       the two sets as the network's forward(x, d) asks for them (one
             kernel call; two vm_reference calls)
  step       one full training step (TensoRFTrainer.train_step on the analytic
             Lego rays, 4096 rays, no density update) on each path

N = 2^18 uniform points in the box, resolution 128 and 300. Every figure is
the median of `--repeats` interleaved rounds after `--warmup` untimed ones,
device events around `--inner` back-to-back calls. The two paths' outputs and
gradients are compared on the way. No GPU: an error, never a CPU figure.

usage: python tools/tensorf_bench.py [--num_samples 262144] [--out profiles/tensorf_bench.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd"), HERE]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from sdf_bench import interleaved  # noqa: E402


def make_sets(res, dev):
    from tensoRF.vm import MAT_IDS, VEC_IDS, line_to_ref, plane_to_ref
    torch.manual_seed(0)
    sets = {}
    for name, R in (("sum16", 16), ("concat48", 48)):
        planes = [(0.1 * torch.randn(res[m1], res[m0], R, device=dev)).requires_grad_() for m0, m1 in MAT_IDS]
        lines = [(0.1 * torch.randn(res[VEC_IDS[i]], R, device=dev)).requires_grad_() for i in range(3)]
        ref = ([plane_to_ref(p.detach()).requires_grad_() for p in planes],
               [line_to_ref(v.detach()).requires_grad_() for v in lines])
        sets[name] = ((planes, lines), ref)
    return sets


def bench_sampling(dev, r, N, args):
    from tensoRF.vm import line_from_ref, plane_from_ref, vm_reference, vm_sample
    res = (r, r, r)
    sets = make_sets(res, dev)
    box = torch.tensor([-1.0, -1, -1, 1, 1, 1], device=dev)
    x = torch.rand(N, 3, device=dev) * 2 - 1
    g_s = torch.randn(N, device=dev)
    g_c = torch.randn(N, 144, device=dev)
    (ks, rs), (kc, rc) = sets["sum16"], sets["concat48"]

    def clear(*groups):
        for planes, lines in groups:
            for t in planes + lines:
                t.grad = None

    def kernel(sigma, color):
        clear(ks, kc)
        s, p = vm_sample(x, box, ks if sigma else None, kc if color else None)
        torch.autograd.backward([t for t in (s, p) if t is not None],
                                [g for g, on in ((g_s, sigma), (g_c, color)) if on])

    def torch_path(sigma, color):
        clear(rs, rc)
        outs, gs = [], []
        if sigma:
            outs.append(vm_reference(x, rs[0], rs[1], "sum", aabb=box)), gs.append(g_s)
        if color:
            outs.append(vm_reference(x, rc[0], rc[1], "concat", aabb=box)), gs.append(g_c)
        torch.autograd.backward(outs, gs)

    def forward_only(path, sigma, color):
        with torch.no_grad():
            if path == "kernel":
                vm_sample(x, box, ks if sigma else None, kc if color else None)
            else:
                if sigma:
                    vm_reference(x, rs[0], rs[1], "sum", aabb=box)
                if color:
                    vm_reference(x, rc[0], rc[1], "concat", aabb=box)

    # the two paths on the way: outputs and gradients
    kernel(True, True)
    torch_path(True, True)
    with torch.no_grad():
        s, p = vm_sample(x, box, ks, kc)
        agree = {"sum_max_abs_diff": float((s - vm_reference(x, rs[0], rs[1], "sum", aabb=box)).abs().max()),
                 "concat_max_abs_diff": float((p - vm_reference(x, rc[0], rc[1], "concat", aabb=box)).abs().max())}
        gd, gm = 0.0, 0.0
        for (kp, kl), (rp, rl) in ((ks, rs), (kc, rc)):
            for a, b in zip(kp, rp):
                gd, gm = max(gd, float((a.grad - plane_from_ref(b.grad)).abs().max())), max(gm, float(b.grad.abs().max()))
            for a, b in zip(kl, rl):
                gd, gm = max(gd, float((a.grad - line_from_ref(b.grad)).abs().max())), max(gm, float(b.grad.abs().max()))
        agree.update(grad_max_abs_diff=gd, grad_max_abs=gm)

    variants = {}
    for name, (sigma, color) in (("sum16", (True, False)), ("concat48", (False, True)), ("both", (True, True))):
        variants[f"{name}_kernel_fwd_bwd"] = lambda s=sigma, c=color: kernel(s, c)
        variants[f"{name}_torch_fwd_bwd"] = lambda s=sigma, c=color: torch_path(s, c)
        variants[f"{name}_kernel_fwd"] = lambda s=sigma, c=color: forward_only("kernel", s, c)
        variants[f"{name}_torch_fwd"] = lambda s=sigma, c=color: forward_only("torch", s, c)
    out = interleaved(variants, args.warmup, args.repeats, args.inner)
    for name in ("sum16", "concat48", "both"):
        for what in ("fwd_bwd", "fwd"):
            out[f"{name}_{what}_torch_over_kernel"] = round(
                out[f"{name}_torch_{what}"]["median_ms"] / out[f"{name}_kernel_{what}"]["median_ms"], 3)
    out.update(agree, resolution=list(res), num_samples=N)
    return out


def bench_step(dev, r, args):
    """One full training step per path, on models with equal weights."""
    from nerf.provider import SyntheticLego, lego_bitfield
    from tensoRF import NeRFNetwork, TensoRFTrainer
    from tensoRF.vm import line_to_ref, plane_to_ref, vm_reference

    class TorchPathNetwork(NeRFNetwork):
        """The same network with the reference's sampling: reference-layout parameters, grid_sample."""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            for name in ("sigma", "color"):
                mats, vecs = getattr(self, f"{name}_mat"), getattr(self, f"{name}_vec")
                setattr(self, f"{name}_mat", nn.ParameterList(nn.Parameter(plane_to_ref(p.data)) for p in mats))
                setattr(self, f"{name}_vec", nn.ParameterList(nn.Parameter(line_to_ref(v.data)) for v in vecs))

        def _vm(self, x, sigma=True, color=True):
            x = x.float()
            s = vm_reference(x, list(self.sigma_mat), list(self.sigma_vec), "sum", aabb=self.aabb_train) \
                if sigma else None
            p = vm_reference(x, list(self.color_mat), list(self.color_vec), "concat", aabb=self.aabb_train) \
                if color else None
            return s, p

    bits = torch.from_numpy(lego_bitfield()).to(dev)
    trainers, samples = {}, {}
    for name, cls in (("kernel", NeRFNetwork), ("torch", TorchPathNetwork)):
        torch.manual_seed(0)
        model = cls(resolution=[r] * 3, bound=1, cuda_ray=True, density_thresh=10).to(dev)
        model.density_bitfield.copy_(bits)
        model.train()
        tr = TensoRFTrainer(model, SyntheticLego(dev, num_rays=4096), iters=30000, update_extra_interval=10 ** 9,
                            log=None)
        tr.global_step = 1  # (no density update: the Lego bitfield stays)
        for _ in range(3):
            tr.train_step()
        k = min(16, model.local_step)
        model.mean_count = int(model.step_counter[:k, 0].sum().item() / k)  # as update_extra_state sets it
        samples[name] = model.mean_count
        trainers[name] = tr
    out = interleaved({f"step_{n}": t.train_step for n, t in trainers.items()}, args.warmup, args.repeats,
                      args.inner)
    out["step_torch_over_kernel"] = round(out["step_torch"]["median_ms"] / out["step_kernel"]["median_ms"], 3)
    out.update(resolution=[r] * 3, num_rays=4096, samples_per_step=samples)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_samples", type=int, default=2 ** 18)
    ap.add_argument("--resolutions", type=int, nargs="*", default=[128, 300])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tensorf_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"median of {args.repeats} interleaved rounds after {args.warmup} warm-up rounds; device events "
                     f"around {args.inner} back-to-back calls; uniform points in the box"}
    for r in args.resolutions:
        res[f"sampling_{r}"] = bench_sampling(dev, r, args.num_samples, args)
        res[f"step_{r}"] = bench_step(dev, r, args)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
