"""CPU: the distortion regulariser's float64 restatement (distortion_helpers)
against the reference's EffDistLoss as recorded in
tests/golden/distortion_reference.npz (tests/golden/make_distortion_golden.py),
the identities the kernels rely on, and the option's argument checks that need
no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import distortion_helpers as dh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distortion_reference.npz")


@pytest.fixture(scope="module")
def cases():
    z = np.load(GOLDEN)
    out = [{k: z[f"c{i}_{k}"] for k in ("w", "m", "interval", "loss", "grad_w")} for i in range(int(z["n_cases"]))]
    assert [c["w"].shape for c in out] == [(1, 1), (1, 2), (1, 7), (1, 64), (1, 65), (1, 257), (1, 64), (3, 7)]
    assert (out[6]["w"][0, 44:] == 0).all() and (out[6]["w"][0, :44] > 0).all()  # the ray with a zero tail
    return out


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def test_restatement_equals_the_reference(cases):
    """Loss (the sum over the rays / n_rays) and its gradient, to 1e-12 relative."""
    for i, c in enumerate(cases):
        B = c["w"].shape[0]
        loss = sum(dh.dist_pairwise(c["w"][b], c["m"][b], c["interval"][b]) for b in range(B)) / B
        grad = np.stack([dh.dist_grad_w(c["w"][b], c["m"][b], c["interval"][b]) for b in range(B)]) / B
        rl, rg = abs(loss - float(c["loss"])) / float(c["loss"]), _rel(grad, c["grad_w"])
        print(f"case {i} {c['w'].shape}: loss {loss:.12e} rel {rl:.2e}, grad rel {rg:.2e}")
        assert float(c["loss"]) > 0 and rl <= 1e-12 and rg <= 1e-12, (i, rl, rg)


def test_gradient_times_weight_sums_to_twice_the_value(cases):
    """dist is homogeneous of degree 2 in w: sum_i g_i w_i = 2 dist (what the
    kernels' backward takes its suffix sums from)."""
    for c in cases:
        for b in range(c["w"].shape[0]):
            w, m, dl = c["w"][b], c["m"][b], c["interval"][b]
            d = dh.dist_pairwise(w, m, dl)
            assert abs(float((dh.dist_grad_w(w, m, dl) * w).sum()) - 2 * d) <= 1e-13 * d


def test_value_is_invariant_under_a_shift_of_m(cases):
    """Only differences of m enter (the kernels subtract the first midpoint)."""
    for c in cases:
        w, m, dl = c["w"][0], c["m"][0], c["interval"][0]
        d = dh.dist_pairwise(w, m, dl)
        for shift in (-m[0], 3.0):
            assert abs(dh.dist_pairwise(w, m + shift, dl) - d) <= 1e-12 * d
            np.testing.assert_allclose(dh.dist_grad_w(w, m + shift, dl), dh.dist_grad_w(w, m, dl), rtol=1e-11, atol=1e-15)


def test_sigma_gradient_equals_autograd():
    """ray_dist's d dist / d sigma against torch autograd (float64) through
    w = alpha T and the pairwise sum, on rays that run to their end, and exact
    zeros behind a stop."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 65):
        deltas = np.stack([rng.uniform(0.003, 0.006, n), rng.uniform(0.001, 0.003, n)], -1)
        sigma = rng.uniform(0.5, 1.5, n) * 3.0 / (n * 0.0045)
        want_d, got = dh.ray_dist(sigma, deltas)
        s = torch.tensor(sigma, dtype=torch.float64, requires_grad=True)
        dl, m = torch.tensor(deltas[:, 0]), torch.tensor(np.cumsum(deltas[:, 1]))
        sd = s * dl
        w = (1 - torch.exp(-sd)) * torch.exp(-(torch.cumsum(sd, 0) - sd))
        d = (w[:, None] * w[None, :] * (m[:, None] - m[None, :]).abs()).sum() + (dl * w * w).sum() / 3
        d.backward()
        assert abs(float(d.detach()) - want_d) <= 1e-12 * want_d
        assert _rel(got, s.grad.numpy()) <= 1e-10, n
    sigma[5] = 1e9
    d, ds = dh.ray_dist(sigma, deltas)
    assert d > 0 and (ds[6:] == 0).all() and (ds[:5] != 0).all()


def test_parser_has_the_flag():
    import main_nerf
    p = main_nerf.get_parser()
    assert p.parse_args(["scene"]).dist_loss_weight == 0.0
    assert p.parse_args(["scene", "--dist_loss_weight", "0.01"]).dist_loss_weight == 0.01


def test_trainers_reject_bad_weights():
    """The checks come before anything touches a device."""
    from types import SimpleNamespace as NS

    from nerf.fused import FusedTrainer
    from nerf.train import Trainer
    # (what the constructor looks at before its option checks)
    model = NS(cuda_ray=True, encoder=NS(level_dim=2, num_levels=16, input_dim=3), sigma_net=NS(input_dim=32),
               color_net=NS(input_dim=32), density_bitfield=torch.zeros(1, dtype=torch.uint8))
    data = NS(num_rays=64)
    with pytest.raises(ValueError, match="dist_loss_weight"):
        FusedTrainer(model, data, M=128, dist_loss_weight=-1.0)
    with pytest.raises(ValueError, match="dist_loss_weight"):
        FusedTrainer(model, data, M=128, dist_loss_weight=float("nan"))
    with pytest.raises(ValueError, match="dist_loss_weight is single-process only"):
        FusedTrainer(model, data, M=128, dist_loss_weight=0.1, distributed=True)
    with pytest.raises(ValueError, match="dist_loss_weight"):
        Trainer(None, None, dist_loss_weight=-0.5)


def test_null_dist_job_is_an_argument_error():
    import _ngp_native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libngp_hip.so not built")
    lib = nat.lib()
    job = nat.DepthLossJob()
    job.color_weight = 1.0
    for entry in (lib.ngp_nerf_composite_loss_dist, lib.ngp_nerf_composite_loss_dist_lists):
        rc = entry(None, None, None, None, None, 0, 0, 1e-4, 1.0, None, 4, None, None, None, None, None, None, None,
                   ctypes.byref(job), None, None)
        assert rc == -1 and b"dist job" in lib.ngp_last_error()
        dj = nat.DistLossJob()
        dj.weight = -1.0
        rc = entry(None, None, None, None, None, 0, 0, 1e-4, 1.0, None, 4, None, None, None, None, None, None, None,
                   ctypes.byref(job), ctypes.byref(dj), None)
        assert rc == -1 and b"weight" in lib.ngp_last_error()
