"""CPU: the background backward's float64 reference (background_helpers.
background_backward64) against torch.autograd, its fp16-faithful form against
the bound the GPU test uses, the rays-list rules, and the conditions the cases
of tests/background_cases.py promise: the route each grid takes, read from its
offsets, and the cap on the rays redrawn for a certain ReLU mask."""
import numpy as np
import pytest
import torch

import background_cases as bc
import background_helpers as bh

NAMES = [c.name for c in bc.CASES]


def _reference(d, saved, **kw):
    x, sph01, bg = saved
    case = bc.BY_NAME[d["name"]] if "name" in d else None
    cw = kw.pop("color_weight", case.color_weight if case else 1.0)
    return bh.background_backward64(x, sph01, bg, d["out_image"], d["out_ws"], d["gt"], d["weights"], bc.SCALE, cw,
                                    d["N"], d["offsets"], d["base"], d["S"], **kw)


def _case(name):
    return dict(bc.case_data(name), name=name)


def test_default_grid_is_the_helpers_default():
    offsets, S = bc.grid_spec(16, 19)
    assert offsets == bh.OFFSETS and S == bh.S and bh.BASE == 16
    x01 = np.random.default_rng(0).random((50, 2))
    table = np.random.default_rng(1).standard_normal((offsets[-1], 2))
    assert np.array_equal(bh.grid64(x01, table), bh.grid64(x01, table, offsets, 16, S))


def test_routes_follow_from_the_offsets():
    """lds0 = (level 0's values <= kLvl0Max); a level is dense where (res + 1)^2
    entries fit; the second loop pass needs more than 64 x 256 rays."""
    lv = {name: bh.grid_levels(*bc.grid_spec(c.base, c.log2T)[:1], c.base, bc.grid_spec(c.base, c.log2T)[1])
          for name, c in bc.BY_NAME.items()}
    scale, res, off0, hs, dense = lv["default"][0]
    assert (res, hs, dense) == (16, 296, True) and 2 * hs <= bc.LVL0_MAX
    assert [l[4] for l in lv["default"]] == [True, True, True, False]
    scale, res, off0, hs, dense = lv["level0_global"][0]
    assert res == 32 and dense and 2 * hs > bc.LVL0_MAX  # level 0 goes through global atomics
    scale, res, off0, hs, dense = lv["level0_hashed"][0]
    assert hs == 256 and hs < 17 ** 2 and not dense and 2 * hs <= bc.LVL0_MAX  # hashed inside the LDS copy
    assert hs & (hs - 1) == 0
    for name in ("second_pass", "second_pass_all"):
        N = bc.BY_NAME[name].N
        assert N == 16384 + 65 and bh.bwd_blocks(N) == 64 and N > 64 * 256
    d = bc.case_data("second_pass")
    assert (d["out_ws"][:bc.ONE_PASS] == 1).all() and (d["out_ws"][bc.ONE_PASS:] < 1).all()
    assert sorted(c.N for c in bc.CASES if c.name.startswith("ragged")) == [1, 63, 64, 65, 255]


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    """Every origin inside the sphere, unit directions, the rays list as the
    case table says, at most 1 % of the rays redrawn and no uncertain unit left
    (the named rays, which cannot be redrawn, included)."""
    case, d = bc.BY_NAME[name], bc.case_data(name)
    N = case.N
    assert d["o"].shape == (N, 3) and float(np.linalg.norm(d["o"], axis=1).max()) < bc.RADIUS
    assert np.allclose(np.linalg.norm(d["d"].astype(np.float64), axis=1), 1, atol=1e-6)
    assert d["redrawn"] <= N // 100, (d["redrawn"], N)
    x, sph01, bg = bc.cpu_saved(d)
    assert not bh.uncertain_units(x, d["weights"]).any()
    assert sph01.min() >= 0 and sph01.max() <= 1 and np.isfinite(bg).all() and float(bg.std()) > 0.1 * (N > 1)
    order = bc.order_of(d)
    if case.rays is None:
        assert order is None
    else:
        inside = order[(order >= 0) & (order < N)]
        assert len(set(inside.tolist())) == inside.size and not np.array_equal(order, np.arange(N))
        if case.rays == "holes":
            assert (order[0::10] == -1).all() and (order[5::10] == N + 3).all() and inside.size == N - len(order[0::5])
        else:
            assert inside.size == N
    if name == "named_rays":
        names, o, dd = bc.named_rays()
        assert d["fixed"] == len(names) == 18 and np.array_equal(d["o"][:18], o)
        x01 = dict(zip(names, sph01[:18].astype(np.float64)))
        assert tuple(x01["+y on the axis"]) == (0.0, 0.5) and tuple(x01["-y on the axis"]) == (1.0, 0.5)
        assert x01["seam +0"][1] == 1.0 and x01["seam -0"][1] == 0.0
        assert x01["centre -x"][1] == 1.0 and x01["centre -x -0"][1] == 0.0
        assert abs(x01["seam + 1e-3"][1] - 1e-3 / (2 * np.pi)) < 1e-6
        assert abs(x01["seam - 1e-3"][1] - (1 - 1e-3 / (2 * np.pi))) < 1e-6
        for k in ("north pole, phi 0.7", "north pole, phi 0.7 - pi"):
            assert abs(x01[k][0] - 1e-3 / np.pi) < 1e-6
        for k in ("south pole, phi 0.7", "south pole, phi 0.7 - pi"):
            assert abs(x01[k][0] - (1 - 1e-3 / np.pi)) < 1e-6


def _autograd(d, x, sph01, bg):
    """scale * cw * mean((base + (1 - ws) * bg(theta) - gt)^2) in float64 torch,
    theta = (table, W0, W1), with the SH columns of x as constants and base
    chosen so that the prediction at theta is out_image."""
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))  # noqa: E731
    table = t(d["table"]).requires_grad_()
    w0, w1 = (t(w).requires_grad_() for w in bh.split_weights(d["weights"]))
    grid = []
    for e, w in bh.grid_corners64(sph01, d["offsets"], d["base"], d["S"]):
        grid.append((t(w)[:, :, None] * table[torch.from_numpy(e)]).sum(1))
    feat = torch.cat([t(x[:, :16]), *grid, torch.zeros(x.shape[0], 8, dtype=torch.float64)], 1)
    assert torch.allclose(feat, t(x), rtol=0, atol=1e-12)
    y = torch.sigmoid(torch.relu(feat @ w0.T) @ w1[:3].T)
    om = (1 - t(d["out_ws"]))[:, None]
    base = t(d["out_image"]) - om * t(bg)
    loss = bc.SCALE * 0.5 * ((base + om * y - t(d["gt"])[:, :3]) ** 2).mean()
    loss.backward()
    return table.grad.numpy(), w0.grad.numpy(), w1.grad.numpy()


@pytest.mark.parametrize("name", ["default", "level0_global", "ragged65"])
def test_reference_equals_autograd(name):
    d = _case(name)
    saved = bc.cpu_saved(d, exact=True)
    got = _reference(d, saved, color_weight=0.5)
    want = _autograd(d, *saved)
    assert np.abs(want[2][3:]).max() == 0
    for what, g, w in zip(("table", "W0", "W1"), got, (want[0], want[1], want[2][:3])):
        assert g.shape == w.shape and np.abs(w).max() > 0
        assert np.abs(g - w).max() <= 1e-10 * np.abs(w).max(), what
    assert (np.abs(got[0]).sum(1) > 0).sum() > 3 * d["N"]  # every level scatters


@pytest.mark.parametrize("name", NAMES)
def test_faithful_stays_within_the_bound(name):
    """The four fp16 roundings move each output by less than the GPU test's
    tolerance. The tolerance's first term takes a rounding as 2^-11 relative,
    which holds for gy, delta and gi in fp16's normal range. At N = 16449 and
    scale 128 (G = 2.6e-3, gy ~ 1e-4) most deltas are fp16 subnormals, rounded
    to 2^-25 absolute instead, and here EVERY value is rounded (on the GPU only
    the few that fall the other way differ), so for those two cases each
    scatter term is allowed that quantum through the rest of the chain:
    2^-25 (1 + A + B), A = max_k sum_u |W0g[u, k]| (a delta's rounding into gi),
    B = max_k sum_u |W0g[u, k]| sum_o |W1[o, u]| (a gy's)."""
    d = _case(name)
    saved, order = bc.cpu_saved(d), bc.order_of(d)
    plain = _reference(d, saved, order=order)
    *faith, b = _reference(d, saved, order=order, faithful=True)
    assert len(plain) == 3 and len(faith) == 3 and b["n_w"] == bh.bwd_blocks(d["N"])
    n_table = b["n_table"][:, None]
    quantum = 0.0
    if name.startswith("second_pass"):
        w0, w1 = (np.abs(w) for w in bh.split_weights(d["weights"]))
        quantum = 2.0 ** -25 * (1 + w0[:, 16:24].sum(0).max() + (w0[:, 16:24] * w1[:3].sum(0)[:, None]).sum(0).max())
    for g, f, S, n, q in zip(plain, faith, (b["S_table"], b["S_w0"], b["S_w1"]), (n_table, b["n_w"], b["n_w"]),
                             (quantum, 0.0, 0.0)):
        assert (np.abs(f - g) <= bh.backward_tolerance(g, S, n) + n * q).all()
    assert int(b["n_table"].sum()) == 16 * _terms(d, saved, order)


def _terms(d, saved, order):
    idx = np.arange(d["N"]) if order is None else order[(order >= 0) & (order < d["N"])]
    sp = saved[1][idx]
    return int(((sp >= 0) & (sp <= 1)).all(1).sum())


def test_rays_list_rules():
    """The identity list is None; a permutation changes nothing beyond the
    order of a float64 sum; holes remove exactly their rays' terms; an entry
    outside [0, 1] in sph01 removes the ray's scatter and nothing else."""
    d = _case("holes")
    saved, N = bc.cpu_saved(d), d["N"]
    none = _reference(d, saved)
    ident = _reference(d, saved, order=np.arange(N, dtype=np.int32))
    perm = _reference(d, saved, order=np.random.default_rng(0).permutation(N))
    for a, b, c in zip(none, ident, perm):
        assert np.array_equal(a, b)
        assert np.abs(a - c).max() <= 1e-12 * np.abs(a).max()
    order = bc.order_of(d)
    gone = np.setdiff1d(np.arange(N), order[(order >= 0) & (order < N)])
    assert gone.size == len(order[0::5])
    holes = _reference(d, saved, order=order)
    only = _reference(d, saved, order=gone)
    for a, h, o in zip(none, holes, only):
        assert np.abs(o).max() > 0
        assert np.abs(a - (h + o)).max() <= 1e-12 * np.abs(a).max()
    x, sph01, bg = saved
    out = sph01.copy()
    out[3, 1], out[7, 0] = np.float32(1.0000001), np.float32(-1e-8)
    moved = _reference(d, (x, out, bg))
    keep = np.setdiff1d(np.arange(N), [3, 7])
    kept = _reference(d, saved, order=keep)
    assert np.array_equal(moved[1], none[1]) and np.array_equal(moved[2], none[2])
    assert np.abs(moved[0] - kept[0]).max() <= 1e-12 * np.abs(none[0]).max()
    assert np.abs(moved[0] - none[0]).max() > 0
