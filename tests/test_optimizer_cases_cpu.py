"""CPU: the optimizer / loss-scaler cases of tests/optimizer_cases.py against
torch alone (torch.amp.GradScaler("cpu"), torch.optim.Adam, LambdaLR), the
float32 restatement's own error (the yardstick of the GPU margin, printed),
and the conditions the cases must satisfy. No GPU."""
import numpy as np
import pytest
import torch

import optimizer_cases as oc

S = oc.SCHEDULE


def _torch_schedule(dtype=torch.float64, n=64):
    """The schedule through torch's own scaler, optimizer and LR schedule.
    -> per update (scale, tracker, adam step, epoch, lr), the final parameter
    and moments, the unscaled fp16 gradients of every update."""
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(n, dtype=dtype) * 0.05)
    p0 = p.detach().clone()
    opt = torch.optim.Adam([p], lr=oc.LR, betas=(oc.B1, oc.B2), eps=oc.EPS)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.1 ** min(it / S["iters"], 1))
    scaler = torch.amp.GradScaler("cpu", init_scale=S["init_scale"], growth_interval=S["growth_interval"])
    rng = np.random.default_rng(5)
    rows, grads = [], []
    for it in range(S["K"]):
        scale = scaler.get_scale() if it else S["init_scale"]
        g16 = (rng.standard_normal(n) * 1e-3 * scale).astype(np.float16)
        if it in S["inf_updates"]:
            g16[(5 * it) % n] = np.inf
        grads.append((g16, scale))
        # the scaled gradient as the backward would leave it: unscale_ divides by the scale
        p.grad = torch.from_numpy(g16.astype(np.float64)).to(dtype)
        scaler.scale(torch.ones(()))  # makes the scaler's scale tensor
        scaler.step(opt)
        scaler.update()
        sched.step()
        step = int(opt.state[p]["step"]) if p in opt.state and "step" in opt.state[p] else 0
        rows.append((scaler.get_scale(), int(scaler._growth_tracker), step, sched.last_epoch, sched.get_last_lr()[0]))
    st = opt.state[p]
    return rows, (p0, p.detach(), st["exp_avg"], st["exp_avg_sq"]), grads


def test_scaler_machine_equals_torch_over_the_schedule():
    """ScalerMachine against torch's GradScaler / Adam / LambdaLR after every
    update, exactly, and both against the literal trajectory; the trajectory
    holds every transition the schedule exists for."""
    rows, _, _ = _torch_schedule()
    mach = oc.ScalerMachine(S["init_scale"], growth_interval=S["growth_interval"])
    for it, row in enumerate(rows):
        skipped = mach.update(int(it in S["inf_updates"]))
        assert skipped == (it in S["inf_updates"])
        scale, tracker, step, epoch, _ = mach.state()
        assert (scale, tracker, step, epoch) == row[:4], (it, mach.state(), row)
        assert mach.iter == it + 1
        # the LR the NEXT update uses (LambdaLR steps after the optimizer), same expression as torch's
        assert mach.lr(oc.LR, S["iters"]) == row[4], (it, mach.lr(oc.LR, S["iters"]), row[4])
        assert tuple(int(x) for x in row[:4]) == oc.TRAJECTORY[it], (it, row)
    assert oc.run_machine() == oc.TRAJECTORY
    assert oc.TRAJECTORY == [
        (65536, 1, 1, 1), (65536, 2, 2, 2), (32768, 0, 2, 3), (32768, 1, 3, 4), (32768, 2, 4, 5), (65536, 0, 5, 6),
        (32768, 0, 5, 7), (16384, 0, 5, 8), (16384, 1, 6, 9), (16384, 2, 7, 10), (32768, 0, 8, 11), (16384, 0, 8, 12),
        (16384, 1, 9, 13), (16384, 2, 10, 14)]
    t = oc.trajectory_transitions(oc.TRAJECTORY)
    assert t["inf_resets_tracker_of_2"] >= 1
    assert t["growths"] == 2 and t["growth_then_backoff"] >= 1
    assert t["backoffs_in_a_row"] >= 1
    assert t["first_lag"] == 2          # adam_step behind epoch from update 2 on
    assert t["clamped_updates"] == 6    # epoch >= iters when the update computes its LR
    assert t["applied"] == 10


def test_scaler_machine_exchange_overflow_and_disabled_scaler():
    """found_inf bit 1 skips without touching scale or tracker; bits 1|2 back
    off; a disabled scaler freezes scale and tracker but counts the steps."""
    m = oc.ScalerMachine(1024.0, growth_interval=3)
    m.update(0), m.update(0)
    assert m.state() == (1024.0, 2, 2, 2, 2)
    assert m.update(2) and m.state() == (1024.0, 2, 2, 3, 3)
    assert not m.update(0) and m.state() == (2048.0, 0, 3, 4, 4)
    assert m.update(3) and m.state() == (1024.0, 0, 3, 5, 5)
    off = oc.ScalerMachine(1024.0, growth_interval=1, enabled=False)
    assert not off.update(0) and off.update(1)
    assert off.state() == (1024.0, 0, 1, 2, 2)
    zero = oc.ScalerMachine(0.0)
    assert zero.unscale_overflows() and zero.update(0) and zero.state() == (0.0, 0, 0, 1, 1)
    sub = oc.ScalerMachine(1e-39)  # a float32 subnormal: 1 / scale overflows float32
    assert sub.unscale_overflows()


def test_adam_reference_equals_torch_adam_float64():
    """adam_reference_f64 against torch.optim.Adam in float64 over the
    schedule (unscaled fp16 gradients cast to float64), to 1e-12 relative."""
    rows, (p0, p_t, m_t, v_t), grads = _torch_schedule(torch.float64)
    mach = oc.ScalerMachine(S["init_scale"], growth_interval=S["growth_interval"])
    p, m, v = p0.numpy().copy(), np.zeros(p0.numel()), np.zeros(p0.numel())
    for it, (g16, scale) in enumerate(grads):
        assert scale == float(mach.scale)
        if it not in S["inf_updates"]:
            p, m, v = oc.adam_reference_f64(p, m, v, g16, scale=scale, step=mach.adam_step + 1,
                                            lr=oc.scheduled_lr(mach.epoch, S["iters"]))
        mach.update(int(it in S["inf_updates"]))
    for name, a, b in (("p", p, p_t), ("m", m, m_t), ("v", v, v_t)):
        b = b.numpy()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name
        assert np.allclose(a, b, rtol=1e-12, atol=0), name


def test_adam_reference_weight_decay_equals_torch():
    torch.manual_seed(1)
    p = torch.nn.Parameter(torch.randn(33, dtype=torch.float64))
    g = torch.randn(33, dtype=torch.float64)
    p0 = p.detach().numpy().copy()
    opt = torch.optim.Adam([p], lr=1e-2, betas=(oc.B1, oc.B2), eps=oc.EPS, weight_decay=0.01)
    m, v, q = np.zeros(33), np.zeros(33), p0
    for step in (1, 2, 3):
        p.grad = g.clone()
        opt.step()
        q, m, v = oc.adam_reference_f64(q, m, v, g.numpy(), step=step, weight_decay=0.01)
    assert np.allclose(q, p.detach().numpy(), rtol=1e-12, atol=0)


LISTS = ["R8", "R4", "R1", "EPS", "RBIG"]


@pytest.mark.parametrize("name", LISTS)
def test_restatement_margin_of_one_update(name, capsys):
    """The float32 restatement of the kernels against the float64 reference on
    each ragged list: max error in ulp32(|ref|) and relative norm per tensor
    kind. These figures (x 4) are the GPU tolerance; the
    bound here only says the restatement is a float32 rounding of the
    reference: rounding the betas to float32 (half an ulp, 3e-8) moves
    1 - beta1 = 0.1 by up to 3e-7 relative and 1 - beta2 = 0.01 by up to 3e-6,
    and with them m and v; the roundings of the arithmetic itself are 6e-8 each."""
    case = oc.make_case(name)
    fig = oc.figures_over_tensors(oc.one_update(case))
    with capsys.disabled():
        print(f"\n[restatement] {name} one update: " +
              ", ".join(f"{k} max {fig[k][0]:.2f} ulp32 rel-norm {fig[k][1]:.2e}" for k in "pmv"))
    for k in "pmv":
        assert fig[k][1] < 5e-6, (name, k, fig[k])
    for gm in (1 / 3, 1 / 8):
        f2 = oc.figures_over_tensors(oc.one_update(case, grad_mult=gm))
        with capsys.disabled():
            print(f"[restatement] {name} grad_mult {gm:.4f}: " +
                  ", ".join(f"{k} max {f2[k][0]:.2f} ulp32 rel-norm {f2[k][1]:.2e}" for k in "pmv"))
        if name == "RBIG":
            break


def test_restatement_margin_of_the_schedule(capsys):
    case = oc.make_case("R4")
    states, pairs = oc.run_schedule(case)
    assert [tuple(int(x) for x in s[:4]) for s in states] == oc.TRAJECTORY
    fig = oc.figures_over_tensors(pairs)
    with capsys.disabled():
        print("\n[restatement] R4 schedule (10 applied updates): " +
              ", ".join(f"{k} max {fig[k][0]:.2f} ulp32 rel-norm {fig[k][1]:.2e}" for k in "pmv"))
    for k in "pmv":
        assert fig[k][1] < 1e-5, (k, fig[k])


def test_restatement_margin_of_adam_step(capsys):
    worst, worst_p = {k: (0.0, 0.0) for k in "pmv"}, 0.0
    for dt, wd, gs, step, n in oc.ADAM_STEP_CASES:
        p, m, v, g = oc.adam_step_inputs(dt, gs, n)
        ref = oc.adam_reference_f64(p, m, v, g, scale=1.0, grad_mult=np.float64(np.float32(gs)), step=step,
                                    weight_decay=wd)
        res = oc.adam_step_restated_f32(p, m, v, g, weight_decay=wd, step=step, grad_scale=gs)
        for i, k in enumerate("pmv"):
            f = oc.error_figures(res[i], ref[i])
            worst[k] = (max(worst[k][0], f[0]), max(worst[k][1], f[1]))
        terms = np.abs(p.astype(np.float64)) + np.abs(ref[0] - p)
        worst_p = max(worst_p, float((np.abs(res[0] - ref[0]) / terms).max()))
    with capsys.disabled():
        print("\n[restatement] ngp_adam_step, worst over its cases: " +
              ", ".join(f"{k} max {worst[k][0]:.2f} ulp32 rel-norm {worst[k][1]:.2e}" for k in "pmv"))
    for k in "mv":
        assert worst[k][1] < 5e-6
    # (p = p0 - update cancels on the one-value cases: its error is held against both terms instead)
    assert worst_p <= 5e-6, worst_p


@pytest.mark.parametrize("name", ["R8", "R4", "R1", "RBIG"])
def test_every_list_has_an_inf_candidate_in_the_scalar_fallback(name):
    case = oc.make_case(name)
    paths = {c: case.nonfinite_path(*c) for c in oc.inf_candidates(case)}
    assert "scalar" in paths.values(), paths
    if name in ("R8", "R4"):
        k = case.misaligned
        assert case.grad_byte_misaligned(k) and (case.off["g"][k] * 2) % 8 == 0
        # a misaligned-only candidate: a full group of 8 that only the pointer sends to the scalar branch
        if case.sizes[k] >= 16:
            assert (k, case.sizes[k] // 2) in paths and case.sizes[k] // 2 // 8 * 8 + 8 <= case.sizes[k]
        assert "vector" in paths.values()
    if name == "RBIG":
        assert case.flat_index(0, case.sizes[0] - 1) >= oc.NONFINITE_CAP  # second trip of the grid-stride loop
    for kind in "pmv":
        assert all((o * 4) % 16 == 0 for o in case.off[kind])
    assert all((o * 2) % 8 == 0 for o in case.off["g"] + case.off["h"])
    assert any(case.has_shadow(k) for k in range(case.n()))
    if name in ("R8", "R4"):
        assert any(not case.has_shadow(k) for k in range(case.n()))


def test_eps_decides_the_update_in_the_eps_case():
    """sqrt(v_hat) within [0.1, 10] x eps, in float64, on at least 64 values."""
    case = oc.make_case("EPS")
    assert case.scale == 2.0 ** 24
    (ref, _), = oc.one_update(case)
    v_hat = ref[2] / (1 - oc.B2)
    r = np.sqrt(v_hat)
    near = (r >= 0.1 * oc.EPS) & (r <= 10 * oc.EPS)
    assert int(near.sum()) >= 64, int(near.sum())
    # ... and there eps moves the update by tens of percent: with eps -> 0 it would be lr exactly
    upd = np.abs(ref[0] - case.view("p", 0).astype(np.float64))[near]
    assert (upd < 0.95 * oc.LR).all() and (upd > 0.05 * oc.LR).all()


@pytest.mark.parametrize("name", ["R4", "RBIG"])
def test_idle_share_of_the_mixed_case(name):
    """Between 25 % and 75 % of the 4-value groups are idle, and idle and
    moved groups alternate (no long run of either)."""
    case = oc.make_case(name)
    idle = np.concatenate(case.groups())
    assert 0.25 <= idle.mean() <= 0.75, idle.mean()
    flips = np.count_nonzero(idle[1:] != idle[:-1])
    assert flips >= idle.size // 4


def test_case_content_and_seams():
    r4, r8 = oc.make_case("R4"), oc.make_case("R8")
    seams = oc.seam_masks(r4.sizes)
    # a whole chunk | a whole chunk + a one-element seam | three chunks + a tail | a short last tensor
    # (tensor 2 starts at flat 4104: 2040 values before its first whole chunk, 9 behind its second)
    assert [int(s.sum()) for s in seams] == [0, 1, 2040 + 9, 12]
    assert all(s.all() for s in oc.seam_masks(r8.sizes))  # every chunk of R8 is a seam
    assert sum(n % 8 != 0 for n in r8.sizes) == len(r8.sizes) - 1 and len(r8.sizes) == oc.K_MAX_TENSORS
    g = np.concatenate([r4.view("g", k) for k in range(r4.n())])
    f = g.view(np.float16).astype(np.float64)
    assert (f > 0).any() and (f < 0).any() and f.max() == 65504.0 and f.min() == -65504.0
    assert (g == 0x8000).any() and (g == 0).any()
    assert np.median(np.abs(f[f != 0])) / r4.scale < 5e-3  # unscaled O(1e-3)
    eps = oc.make_case("EPS")
    assert (eps.view("g", 0) == 0x0001).sum() >= 64 and (eps.view("g", 0) == 0x8001).sum() >= 64
    packed = oc.make_case("R8", packed=True)
    st = oc.flat_starts(packed.sizes)
    assert [o - packed.off["g"][0] for o in packed.off["g"]] == st[:-1]
    assert int(packed.padding.sum()) == st[-1] - sum(packed.sizes)
    for case in (r4, r8, packed):
        for kind in "pmvgh":
            assert case.canary[kind][:oc.GUARD].all() and case.canary[kind][-oc.GUARD:].all()
