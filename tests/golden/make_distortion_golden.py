"""Generates tests/golden/distortion_reference.npz from the reference's own
EffDistLoss (loss.py:29-76), executed from its file in float64 on the CPU (the
fixture is data and travels, the reference does not). Usage:
    python tests/golden/make_distortion_golden.py <reference checkout>

Cases `c0..c7`, each with w, m, interval [B, n], the reference's loss (the sum
over the B rays divided by B) and its gradient with respect to w for a unit
output gradient: single rays of 1, 2, 7, 64, 65 and 257 samples, a 64-sample
ray whose last 20 weights are zero (a ray that stopped early), and a batch of
3 rays of 7 samples (the / n_rays).
The rays are shaped as the training march makes them: weights of a composite
(alpha_i T_i of random densities), midpoints increasing from a first one at
0.3, intervals of a few thousandths.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(ref, "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.eff_distloss


def make_rays(rng, B, n, zero_tail=0):
    interval = rng.uniform(0.003, 0.006, (B, n))
    step = rng.uniform(0.001, 0.003, (B, n))
    step[:, 0] = 0.3
    m = np.cumsum(step, -1)
    sigma = rng.uniform(0.5, 1.5, (B, n)) * 3.0 / (n * 0.0045)
    sd = sigma * interval
    T = np.exp(-(np.cumsum(sd, -1) - sd))
    w = (1 - np.exp(-sd)) * T
    if zero_tail:
        w[:, n - zero_tail:] = 0.0
    return w, m, interval


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    eff_distloss = load_reference(sys.argv[1])
    rng = np.random.default_rng(29)
    out = {}
    shapes = [(1, 1, 0), (1, 2, 0), (1, 7, 0), (1, 64, 0), (1, 65, 0), (1, 257, 0), (1, 64, 20), (3, 7, 0)]
    for k, (B, n, tail) in enumerate(shapes):
        w, m, interval = make_rays(rng, B, n, tail)
        tw = torch.from_numpy(w).requires_grad_(True)
        loss = eff_distloss(tw, torch.from_numpy(m), torch.from_numpy(interval))
        loss.backward()
        assert loss.dtype == torch.float64
        out[f"c{k}_w"], out[f"c{k}_m"], out[f"c{k}_interval"] = w, m, interval
        out[f"c{k}_loss"] = np.float64(loss.item())
        out[f"c{k}_grad_w"] = tw.grad.numpy()
    out["n_cases"] = np.int64(len(shapes))
    path = os.path.join(HERE, "distortion_reference.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {len(shapes)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
