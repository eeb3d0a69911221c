"""GPU: early ray termination in the reference-API compositing kernels and in
the render loops, against the CPU oracle (cases: tests/composite_cases.py,
checked without a GPU in tests/test_composite_cases_cpu.py).

  * k_composite_train_fwd / k_composite_train_bwd (one wave per ray, 64-sample
    chunks): rays whose T crosses T_thresh on either side of a chunk edge, in
    a shuffled ray table with N % 4 != 0, empty and overflow rays. Every output
    buffer starts as NaN, so a row the kernel skips or should not have written
    shows.
  * k_march_rays / k_composite_rays in the reference's host loop, and
    k_render_init / k_render_march / k_render_composite driven directly, over a
    synthetic field evaluated on the host from the read-back positions: both
    against the oracle's loop, iteration by iteration.
"""
import numpy as np
import pytest
import torch

import composite_cases as cc

pytestmark = pytest.mark.gpu

TRAIN = [(v, T) for v in cc.VARIANTS for T in cc.T_THRESHES]
NAN = float("nan")


def t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a copy: the cases are read-only)


def _forward(cuda, c):
    import raymarching.backend as rb
    N, M = c["N"], c["M"]
    ins = [t(c[k], cuda) for k in ("sigmas", "rgbs", "deltas", "rays")]
    ws, dp, img = (torch.full((N,), NAN, device=cuda), torch.full((N,), NAN, device=cuda),
                   torch.full((N, 3), NAN, device=cuda))
    rb._backend.composite_rays_train_forward(*ins, M, N, c["T_thresh"], ws, dp, img)
    return ins, (ws, dp, img)


def _backward(cuda, c, fill=NAN):
    import raymarching.backend as rb
    N, M = c["N"], c["M"]
    ins, outs = _forward(cuda, c)
    gs, gc = torch.full((M,), fill, device=cuda), torch.full((M, 3), fill, device=cuda)
    rb._backend.composite_rays_train_backward(t(c["gws"], cuda), t(c["gdepth"], cuda), t(c["gimage"], cuda), *ins,
                                              *outs, M, N, c["T_thresh"], gs, gc)
    return gs.cpu().numpy(), gc.cpu().numpy()


def _check_forward(c, r, ws, dp, img):
    idx = c["rays"][:, 0]
    for got, ref in ((ws, r["ws"]), (dp, r["depth"]), (img, r["image"])):
        assert not np.isnan(got).any()            # all N rows written
        assert (got[idx[~c["valid"]]] == 0).all()  # empty and overflow rays: exact zeros
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)


def _check_backward(c, r, gs, gc):
    stop, solid = cc.last_written(gs, gc, c["rays"], c["valid"])
    # the last row the kernel wrote is the oracle's stop sample, on every ray ...
    bad = np.flatnonzero(stop != r["stop"])
    assert bad.size == 0, [(int(c["kind"][n]), int(c["rays"][n, 2]), int(c["kstar"][n]), float(c["eps"][n]),
                            int(stop[n]), int(r["stop"][n])) for n in bad[:8]]
    # ... every row up to it is written in both buffers, every row past it and every row of an
    # empty / overflow ray still holds the sentinel (the reference leaves them untouched)
    assert solid.all(), np.flatnonzero(~solid)
    assert np.array_equal(np.isnan(gs), np.isnan(r["grad_sigmas"]))
    assert np.array_equal(np.isnan(gc), np.isnan(r["grad_rgbs"]))
    w = ~np.isnan(r["grad_sigmas"])
    np.testing.assert_allclose(gc[w], r["grad_rgbs"][w], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gs[w], r["grad_sigmas"][w], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("variant,T_thresh", TRAIN)
def test_composite_train_forward_early_stop(cuda, variant, T_thresh):
    c, r = cc.train_case(variant, T_thresh), cc.train_reference(variant, T_thresh)
    _, outs = _forward(cuda, c)
    _check_forward(c, r, *[a.cpu().numpy() for a in outs])


@pytest.mark.parametrize("variant,T_thresh", TRAIN)
def test_composite_train_backward_stop_rows(cuda, variant, T_thresh):
    c, r = cc.train_case(variant, T_thresh), cc.train_reference(variant, T_thresh)
    _check_backward(c, r, *_backward(cuda, c))


@pytest.mark.parametrize("T_thresh", cc.T_THRESHES)
def test_composite_train_autograd_function(cuda, T_thresh):
    """raymarching.composite_rays_train: the same values, and (its gradient
    buffers start as zeros) exact zeros past the stop sample and on the rows of
    the rays it does not composite."""
    import raymarching
    c, r = cc.train_case(2, T_thresh), cc.train_reference(2, T_thresh)
    sig = t(c["sigmas"], cuda).requires_grad_(True)
    rgb = t(c["rgbs"], cuda).requires_grad_(True)
    ws, dp, img = raymarching.composite_rays_train(sig, rgb, t(c["deltas"], cuda), t(c["rays"], cuda), T_thresh)
    _check_forward(c, r, *[a.detach().cpu().numpy() for a in (ws, dp, img)])
    torch.autograd.backward([ws, dp, img], [t(c["gws"], cuda), t(c["gdepth"], cuda), t(c["gimage"], cuda)])
    gs, gc = sig.grad.cpu().numpy(), rgb.grad.cpu().numpy()
    w = ~np.isnan(r["grad_sigmas"])
    assert (gs[~w] == 0).all() and (gc[~w] == 0).all()
    assert w.sum() < c["M"] - 1000  # (the early stops leave a good part of the rows out)
    np.testing.assert_allclose(gc[w], r["grad_rgbs"][w], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gs[w], r["grad_sigmas"][w], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("T_thresh", cc.T_THRESHES)
def test_composite_train_backward_vs_float64(cuda, parity_report, T_thresh):
    """Against torch-CPU float64 autograd of the plain compositing formula over
    the oracle's stop set (a formula error the oracle shared would show): the
    kernel within 4x the fp32 oracle's own error against the same reference
    (the factor: expf differing in the last place, fma contraction). Measured
    oracle errors: grad_sigmas max abs 5.5e-9 / 7.8e-9, per entry over |ref| +
    1e-3 max |ref| 2.0e-4 / 2.4e-4, grad_rgbs max abs 9.4e-8 / 1.8e-7 at
    T_thresh 1e-4 / 1e-2; the kernel's are in the parity summary."""
    c, r = cc.train_case(1, T_thresh), cc.train_reference(1, T_thresh)
    ref = cc.float64_backward(c, r["stop"])
    orc = cc.float64_errors(r["grad_sigmas"], r["grad_rgbs"], ref)
    gs, gc = _backward(cuda, c)
    assert np.array_equal(~np.isnan(gs), ref[2])
    got = cc.float64_errors(gs, gc, ref)
    parity_report(f"T_thresh {T_thresh:g}: vs float64 (grad_sigmas max abs, per entry scaled, grad_rgbs max abs) "
                  f"oracle {orc[0]:.2e} {orc[1]:.2e} {orc[2]:.2e}, kernel {got[0]:.2e} {got[1]:.2e} {got[2]:.2e}")
    print("float64 errors: oracle", orc, "kernel", got)
    for g, o in zip(got, orc):
        assert g <= 4 * o, (got, orc)


# ------------------------------------------------------------------ render loops

def _loop_device_inputs(cuda, inp):
    return {k: t(inp[k], cuda) for k in ("rays_o", "rays_d", "nears", "fars", "bits", "noises")}


def _check_final(inp, o, ws, dp, img, death_iter):
    ok = ~o["near"]
    for got, ref in ((ws, o["weights_sum"]), (dp, o["depth"]), (img, o["image"])):
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-5, atol=1e-6)
    # a near-threshold ray may stop one sample earlier or later
    assert (np.abs(img[~ok] - o["image"][~ok]) <= 2 * inp["T_thresh"]).all()
    assert (np.abs(death_iter[~ok] - o["death_iter"][~ok]) <= 1).all()
    assert np.array_equal(death_iter[ok], o["death_iter"][ok])


@pytest.mark.parametrize("name", sorted(cc.LOOP_CONFIGS))
def test_op_surface_loop_matches_oracle_loop(cuda, parity_report, name):
    """The reference's host loop (renderer.py:384-420) over _backend.march_rays
    / _backend.composite_rays with torch compaction: per iteration the samples
    are bit-equal, the alive list after the composite is equal (so every ray
    stops on the oracle's sample: T = 1 - weight_sum tested before the sample
    is added, a ray dying on the sample that fills its n_step), rays_t is
    written for the survivors only."""
    import raymarching.backend as rb
    inp, o = cc.loop_inputs(name), cc.oracle_loop(name)
    assert not o["near"].any()  # (the cases hold no near-threshold ray: every list below is compared whole)
    N, d = inp["N"], _loop_device_inputs(cuda, inp)
    ws, dp, img = torch.zeros(N, device=cuda), torch.zeros(N, device=cuda), torch.zeros(N, 3, device=cuda)
    alive = torch.arange(N, dtype=torch.int32, device=cuda)
    rays_t = d["nears"].clone()
    death_iter = np.full(N, -1)
    step, i = 0, 0
    while step < inp["max_steps"]:
        n_alive = alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        it = o["iters"][i]
        assert (n_alive, n_step, step) == (it["n_alive"], it["n_step"], it["step"])
        Mi = n_alive * n_step
        xyzs, dirs, deltas = (torch.zeros(Mi, 3, device=cuda), torch.zeros(Mi, 3, device=cuda),
                              torch.zeros(Mi, 2, device=cuda))
        noises = d["noises"][:n_alive].contiguous() if step == 0 else torch.zeros(n_alive, device=cuda)
        rb._backend.march_rays(n_alive, n_step, alive, rays_t, d["rays_o"], d["rays_d"], inp["bound"],
                               inp["dt_gamma"], inp["max_steps"], inp["C"], cc.GRID_H, d["bits"], d["nears"],
                               d["fars"], xyzs, dirs, deltas, noises)
        x = xyzs.cpu().numpy()
        assert np.array_equal(x.view(np.uint32), it["xyzs"].view(np.uint32))
        assert np.array_equal(deltas.cpu().numpy().view(np.uint32), it["deltas"].view(np.uint32))
        sigma, logits = cc.field(x)
        before = alive.cpu().numpy()
        rb._backend.composite_rays(n_alive, n_step, inp["T_thresh"], alive, rays_t, t(sigma, cuda),
                                   t(cc.sigmoid_h(logits), cuda), deltas, ws, dp, img)
        after = alive.cpu().numpy()
        assert np.array_equal(after, it["alive_after"])
        assert np.array_equal(rays_t.cpu().numpy().view(np.uint32), it["rays_t"].view(np.uint32))
        np.testing.assert_allclose(ws.cpu().numpy(), it["weights_sum"], rtol=1e-5, atol=1e-6)
        death_iter[before[after < 0]] = i
        alive = alive[alive >= 0]
        step += n_step
        i += 1
    assert i == len(o["iters"]) and step == o["step"]
    assert np.array_equal(alive.cpu().numpy(), o["alive_end"])
    _check_final(inp, o, ws.cpu().numpy(), dp.cpu().numpy(), img.cpu().numpy(), death_iter)
    parity_report(f"config {name}: {i} iterations, {(o['cause'] == cc.BY_T).sum()} rays ended by T, "
                  f"{(o['cause'] == cc.RAN_OUT).sum()} ran out, {alive.shape[0]} alive at the end")


@pytest.mark.parametrize("name,null_noises", [("a", False), ("b", False), ("c", True), ("d", False)],
                         ids=["a", "b", "c-null-noises", "d"])
def test_device_loop_matches_oracle_loop(cuda, name, null_noises):
    """ngp_render_init / ngp_render_march / ngp_render_composite driven
    directly (no network: sigma and the colour logits come from the field, on
    the host): per iteration the state slot (count, n_alive, step), the samples
    of every ray with the rows past its last sample zeroed, the set of the
    next alive list and rays_t are the oracle loop's; iterations past the end
    are no-ops; a null noises pointer means no noise."""
    import _ngp_native as nat
    inp, o = cc.loop_inputs(name), cc.oracle_loop(name)
    assert not o["near"].any() and not (null_noises and inp["noise"])
    N, d = inp["N"], _loop_device_inputs(cuda, inp)
    lib, P = nat.lib(), nat.ptr
    s = nat.stream_of(d["rays_o"])
    f = lambda *shape: torch.full(shape, NAN, device=cuda)  # noqa: E731
    alive = [torch.full((N,), -7, dtype=torch.int32, device=cuda) for _ in range(2)]
    rays_t, ws, dp, img = f(N), f(N), f(N), f(N, 3)
    xyzs, dirs, deltas = f(N, 3), f(N, 3), f(N, 2)
    sigma = torch.zeros(N, device=cuda)
    color = torch.zeros(N, 16, dtype=torch.float16, device=cuda)
    state = torch.zeros(int(lib.ngp_render_state_bytes()), dtype=torch.uint8, device=cuda)
    assert state.numel() == 32
    slots = lambda: state.view(torch.int32).cpu().numpy().reshape(2, 4)  # noqa: E731  {count, n_alive, step, pad}
    nat.check(lib.ngp_render_init(N, P(d["nears"]), P(alive[0]), P(rays_t), P(ws), P(dp), P(img), P(state), s),
              "render_init")
    assert np.array_equal(alive[0].cpu().numpy(), np.arange(N))
    assert torch.equal(rays_t.view(torch.int32), d["nears"].view(torch.int32))  # (bits: a near may be NaN)
    assert not ws.any() and not dp.any() and not img.any()
    assert np.array_equal(slots(), [[0, N, 0, 0], [0, 0, 0, 0]])
    noises = None if null_noises else d["noises"]
    death_iter = np.full(N, -1)
    iters = o["iters"]
    for i in range(len(iters) + 3):
        cur, nxt = alive[i & 1], alive[(i + 1) & 1]
        for b in (xyzs, dirs, deltas):
            b.fill_(NAN)
        nat.check(lib.ngp_render_march(N, i, P(state), P(cur), P(rays_t), P(d["rays_o"]), P(d["rays_d"]),
                                       inp["bound"], inp["dt_gamma"], inp["max_steps"], inp["C"], cc.GRID_H,
                                       P(d["bits"]), P(d["fars"]), P(xyzs), P(dirs), P(deltas), P(noises), s),
                  "render_march")
        st = slots()
        if i < len(iters):
            it = iters[i]
            n_alive, n_step = it["n_alive"], it["n_step"]
            count = n_alive * n_step
            assert list(st[i & 1][:3]) == [count, n_alive, it["step"]]
            assert list(st[(i + 1) & 1][:3]) == [0, 0, it["step"] + n_step]
            listed = cur[:n_alive].cpu().numpy()
            order = np.argsort(it["alive"], kind="stable")
            row = order[np.searchsorted(it["alive"][order], listed)]  # the oracle's row of each listed ray
            assert np.array_equal(it["alive"][row], listed)           # (the same set, in any order)
            x = xyzs.cpu().numpy()
            dl = deltas.cpu().numpy()
            assert np.array_equal(x[:count].reshape(n_alive, n_step, 3).view(np.uint32),
                                  it["xyzs"].reshape(n_alive, n_step, 3)[row].view(np.uint32))
            assert np.array_equal(dl[:count].reshape(n_alive, n_step, 2).view(np.uint32),
                                  it["deltas"].reshape(n_alive, n_step, 2)[row].view(np.uint32))
            assert np.isnan(x[count:]).all() and np.isnan(dl[count:]).all()
            assert not np.isnan(dirs[:count].cpu().numpy()).any()
            sg, logits = cc.field(x[:count])
            sigma[:count] = t(sg, cuda)
            color[:count, :3] = t(logits, cuda)
        else:  # a spare iteration
            assert st[i & 1][0] == 0 and np.isnan(xyzs.cpu().numpy()).all()
            keep = [a.clone() for a in (rays_t, ws, dp, img)]
        nat.check(lib.ngp_render_composite(N, i, inp["max_steps"], P(state), inp["T_thresh"], P(cur), P(nxt),
                                           P(rays_t), P(sigma), P(color), P(deltas), P(ws), P(dp), P(img), s),
                  "render_composite")
        if i < len(iters):
            survivors = it["alive_after"][it["alive_after"] >= 0]
            st = slots()
            assert list(st[(i + 1) & 1][:3]) == [0, survivors.size, it["step"] + n_step]
            assert np.array_equal(np.sort(nxt[:survivors.size].cpu().numpy()), np.sort(survivors))
            assert np.array_equal(rays_t.cpu().numpy().view(np.uint32), it["rays_t"].view(np.uint32))
            np.testing.assert_allclose(ws.cpu().numpy(), it["weights_sum"], rtol=1e-5, atol=1e-6)
            death_iter[np.setdiff1d(it["alive"], survivors)] = i
        else:
            for a, b in zip(keep, (rays_t, ws, dp, img)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _check_final(inp, o, ws.cpu().numpy(), dp.cpu().numpy(), img.cpu().numpy(), death_iter)
