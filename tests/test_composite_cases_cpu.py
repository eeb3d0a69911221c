"""The early-termination cases of tests/composite_cases.py do what they claim
(no GPU): checked with the CPU oracle alone, so tests/test_gpu_composite.py can
demand the identical stop sample / alive list from the device."""
import numpy as np
import pytest

import composite_cases as cc

TRAIN = [(v, T) for v in cc.VARIANTS for T in cc.T_THRESHES]


@pytest.mark.parametrize("variant,T_thresh", TRAIN)
def test_train_cases_cover_the_early_stop(variant, T_thresh):
    c = cc.train_case(variant, T_thresh)
    r = cc.train_reference(variant, T_thresh)
    rays, kind, valid = c["rays"], c["kind"], c["valid"]
    N, M = c["N"], c["M"]
    assert 60 <= N <= 100 and N % 4 == variant and M < 20000
    assert sorted(rays[:, 0]) == list(range(N)) and not np.array_equal(rays[:, 0], np.arange(N))
    # every length with every crossing that fits, each sign and size of eps, and a ray that never stops
    for length in cc.LENGTHS:
        sel = (kind == cc.CROSS) & (rays[:, 2] == length)
        assert sorted(c["kstar"][sel]) == cc.crossings(length)
        assert ((kind == cc.NEVER) & (rays[:, 2] == length)).sum() == 1
    assert {(abs(e), np.sign(e)) for e in c["eps"][kind == cc.CROSS]} == \
        {(1e-3, 1.0), (1e-3, -1.0), (1e-2, 1.0), (1e-2, -1.0)}
    assert (kind == cc.EMPTY).sum() >= 2 and (rays[kind == cc.EMPTY, 2] == 0).all()
    over = kind == cc.OVERFLOW
    assert over.sum() == 2 and (rays[over, 1].astype(np.int64) + rays[over, 2] > M).all() and (rays[over, 2] > 0).all()
    assert not valid[over].any() and not valid[kind == cc.EMPTY].any() and valid.sum() == N - over.sum() - (kind == cc.EMPTY).sum()
    for k in (cc.ZERO,):
        for n in np.flatnonzero(kind == k):
            assert (c["sigmas"][rays[n, 1]:rays[n, 1] + rays[n, 2]] == 0).all()
    inf_ray, big_ray = np.flatnonzero(kind == cc.INF)[0], np.flatnonzero(kind == cc.BIG)[0]
    assert np.isinf(c["sigmas"][rays[inf_ray, 1] + c["kstar"][inf_ray]])
    assert c["sigmas"][rays[big_ray, 1] + c["kstar"][big_ray]] == np.float32(1e9)
    # the valid rays' rows are disjoint and the first overflow ray owns the rows it has inside the buffer
    owner = np.zeros(M, int)
    for n in np.flatnonzero(valid | over):
        owner[rays[n, 1]:min(rays[n, 1] + rays[n, 2], M)] += 1
    assert (owner == 1).all()

    stop, fired, margin = cc.serial_stop(c)
    # the oracle (rows it wrote over a NaN fill) and the fp32 restatement agree on every ray's stop ...
    assert np.array_equal(stop, r["stop"])
    # ... and at every crossing the serial T clears T_thresh by more than 1e-4 (relative) on both
    # sides: a kernel whose expf differs in the last place has to stop on the same sample
    assert (margin[fired] > 1e-4).all(), margin[fired].min()
    length = rays[:, 2]
    early = fired & (stop < length - 1)
    assert early.sum() * 3 >= N, (early.sum(), N)
    assert (fired & (stop % 64 == 63)).sum() >= 5                    # the chunk's last lane
    assert (fired & (stop % 64 == 0) & (stop >= 64)).sum() >= 5      # lane 0 of a later chunk
    assert not fired[kind == cc.NEVER].any() and not fired[kind == cc.ZERO].any()
    assert stop[inf_ray] == c["kstar"][inf_ray] and stop[big_ray] == c["kstar"][big_ray] == 64
    # alpha = 0 and the empty / overflow rays in the oracle's outputs
    idx = rays[:, 0]
    for a in (r["ws"], r["depth"], r["image"]):
        assert np.isfinite(a).all()
        assert (a[idx[~valid]] == 0).all() and (a[idx[kind == cc.ZERO]] == 0).all()
    assert abs(r["ws"][idx[inf_ray]] - 1) < 1e-6 and abs(r["ws"][idx[big_ray]] - 1) < 1e-6


@pytest.mark.parametrize("T_thresh", cc.T_THRESHES)
def test_train_oracle_against_float64(T_thresh):
    """The fp32 oracle's backward against float64 autograd of the plain formula
    over the oracle's stop set: the errors the GPU test scales its bound from
    (measured: grad_sigmas max abs 5.5e-9 / 7.8e-9 and per entry over |ref| +
    1e-3 max |ref| 2.0e-4 / 2.4e-4, grad_rgbs max abs 9.4e-8 / 1.8e-7 at
    T_thresh 1e-4 / 1e-2)."""
    c, r = cc.train_case(1, T_thresh), cc.train_reference(1, T_thresh)
    ref = cc.float64_backward(c, r["stop"])
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    assert ref[2].sum() == (r["stop"][c["valid"]] + 1).sum()
    abs_s, rel_s, abs_c = cc.float64_errors(r["grad_sigmas"], r["grad_rgbs"], ref)
    assert abs_s <= 5e-8 and rel_s <= 1e-3 and abs_c <= 1e-6, (abs_s, rel_s, abs_c)
    assert np.abs(ref[0]).max() > 1e-3  # (the gradients are not all tiny)


def test_field_is_exact_and_its_sigmoid_robust():
    """The synthetic field takes few values, all exact in their formats, and no
    colour logit's sigmoid sits where the last place of expf decides its half
    rounding (so the device's sigmoid gives the same half)."""
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-2, 2, (20000, 3)).astype(np.float32)
    sigma, logits = cc.field(xyz)
    assert sigma.dtype == np.float32 and logits.dtype == np.float16
    assert (sigma == 0).mean() > 0.3 and (sigma == cc.SIGMA_SOLID).mean() > 0.03
    ramp = sigma[(sigma > 0) & (sigma < cc.SIGMA_SOLID)]
    assert ramp.size > 5000 and 100 < ramp.max() <= cc.SIGMA_RAMP
    assert len(np.unique(ramp)) > 0.9 * ramp.size  # (no plateau: expf sees no argument twice)
    assert np.array_equal(sigma, cc.field(xyz.copy())[0])
    assert np.array_equal(logits.astype(np.float64), np.stack([cc.LOGITS[(cc._hash(xyz) >> s) & 0xff]
                                                                 for s in (8, 16, 24)], -1))
    assert len(np.unique(logits)) == 256
    x = cc.LOGITS.astype(np.float16)
    exact = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    assert np.array_equal(cc.sigmoid_h(x), exact.astype(np.float16).astype(np.float32))
    h = exact.astype(np.float16).astype(np.float64)
    half_ulp = np.spacing(exact.astype(np.float16)).astype(np.float64) / 2
    to_tie = np.abs(np.abs(exact - h) - half_ulp)        # distance to the nearest rounding boundary
    assert (to_tie > 8 * np.spacing(exact.astype(np.float32))).all()


def test_loop_case_d_holds_the_degenerate_rays():
    """Configuration d (rays of tests/ray_cases.py) meets every claim below,
    and on top of them: cameras inside the box, exact zeros in directions, NaN
    near and NaN far, rays pointing away and rays that miss. The loop starts
    them all at rays_t = near; those that can take no sample leave in the
    first iteration without one and without a rays_t."""
    inp, o = cc.loop_inputs("d"), cc.oracle_loop("d")
    nears, fars = inp["nears"], inp["fars"]
    fmax = np.finfo(np.float32).max
    nan, miss = np.isnan(nears) | np.isnan(fars), fars == fmax
    away = ~nan & ~miss & (fars < nears)
    assert np.isnan(nears).sum() >= 2 and np.isnan(fars).sum() >= 2 and miss.sum() >= 64 and away.sum() >= 64
    assert ((inp["rays_d"] == 0).sum(1) == 2).sum() >= 64 and np.signbit(inp["rays_d"][inp["rays_d"] == 0]).any()
    assert (np.abs(inp["rays_o"]) <= inp["bound"]).all(1).sum() >= 128
    dead = nan | miss | away
    assert (o["death_iter"][dead] == 0).all() and (o["samples"][dead] == 0).all()
    assert (o["cause"][dead] == cc.RAN_OUT).all()
    first = o["iters"][0]
    assert (first["alive_after"][dead] == -1).all()
    assert np.array_equal(first["rays_t"][dead].view(np.uint32), nears[dead].view(np.uint32))
    assert (o["samples"][~dead] > 0).sum() >= 100
    assert (o["death_iter"] > 0).sum() >= 100  # the loop goes on past the first iteration for the rest


@pytest.mark.parametrize("name", sorted(cc.LOOP_CONFIGS))
def test_loop_cases_cover_both_endings(name):
    inp, o = cc.loop_inputs(name), cc.oracle_loop(name)
    N = inp["N"]
    cause = o["cause"]
    assert (cause == cc.BY_T).sum() >= 0.05 * N, (cause == cc.BY_T).sum()
    assert (cause == cc.RAN_OUT).sum() >= 0.05 * N, (cause == cc.RAN_OUT).sum()
    if name == "c":
        assert o["step"] >= inp["max_steps"] and (cause == cc.ALIVE).sum() > 0
        assert np.array_equal(np.sort(o["alive_end"]), np.flatnonzero(cause == cc.ALIVE))
    else:
        assert o["step"] < inp["max_steps"] and o["alive_end"].size == 0 and (cause != cc.ALIVE).all()
    assert len({it["n_step"] for it in o["iters"]}) > 2
    assert (o["weights_sum"] > 0).mean() >= 0.3
    assert o["near"].sum() <= 0.02 * N, o["near"].sum()
    # (in fact none with this field, so the GPU tests compare every alive list whole)
    assert not o["near"].any()
    # a ray that dies on the very sample that fills its n_step, and rays_t kept for the dead
    filled = 0
    for it in o["iters"]:
        if it["n_step"] > 1:
            d0 = it["deltas"].reshape(it["n_alive"], it["n_step"], 2)[:, :, 0]
            filled += int(((it["alive_after"] < 0) & (d0 != 0).all(1)).sum())
    assert filled > 0
    if inp["noise"]:
        assert (inp["noises"] > 0).any()
    assert np.isfinite(o["image"]).all() and np.isfinite(o["depth"]).all()
