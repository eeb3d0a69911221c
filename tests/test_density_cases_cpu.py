"""CPU: tests/density_cases.py proved against something other than itself.

  * points_ref against torch-CPU evaluating the reference's expressions
    (nerf/renderer.py:524-533), bit for bit. One operation needs care: the
    reference runs `2 * coords.float() / (H - 1)` on the device, where torch
    divides a tensor by a Python scalar as a multiplication by the scalar's
    fp32 reciprocal (that is what k_density_points and points_ref restate);
    torch-CPU divides truly, and the two differ by an ulp for some cells once
    H - 1 is not a power of two (6 of 16 coordinates at H = 16, 8 of 128 at
    H = 128). So the expressions are evaluated twice: with the division
    written as the device performs it, bit for bit at every H and bound; and
    literally, bit for bit at H = 2 and 4 (every coordinate: the two divisions
    agree on all of them), and at H = 16 and 128 within 12 * 2^-24 * bound,
    which bounds what one ulp of the quotient can become: the quotient's two
    forms differ by at most 3 roundings of a value <= 2 (6 * 2^-24), the
    subtraction adds one rounding of a value <= 1 on each side (8), the scale
    <= bound one on each side (10 * bound), the final add likewise (12 * bound).
  * ema_pack_ref (with points_ref and run_max_ref before it) replaying the
    reference-executed fixture's updates u0..u3 on the analytic field, to
    test_density_golden.py's tolerance.
  * every case table against the conditions it exists for.
"""
import math

import numpy as np
import pytest
import torch

import density_cases as dc
import oracle
from test_density_golden import CASES, RTOL, _bits_match, _draws, _fixture

F32 = np.float32


def _torch_points(coords, noise, H, bound_c, literal):
    """renderer.py:524 / :528-533 on torch-CPU for one cascade."""
    c = torch.from_numpy(coords)
    if literal:
        xyzs = 2 * c.float() / (H - 1) - 1
    else:  # tensor / scalar as the device kernel does it: times the fp32 reciprocal
        xyzs = 2 * c.float() * (torch.tensor(1.0) / torch.tensor(float(H - 1))) - 1
    hgs = bound_c / H
    cas_xyzs = xyzs * (bound_c - hgs)
    cas_xyzs += (torch.from_numpy(noise) * 2 - 1) * hgs
    return cas_xyzs.numpy()


@pytest.mark.parametrize("bound", [1, 2, 3, 16])
@pytest.mark.parametrize("H", [2, 4, 16, 128])
def test_points_ref_matches_torch_cpu(H, bound):
    C = 1 + math.ceil(math.log2(bound))
    rng = np.random.default_rng(100 * H + bound)
    ppc = 4096
    coords = rng.integers(0, H, (C * ppc, 3)).astype(np.int32)
    coords[:H] = np.arange(H, dtype=np.int32)[:, None]  # every coordinate value, the corners among them
    noise = rng.random((C * ppc, 3)).astype(F32)
    noise[0], noise[1] = 0.0, F32(1 - 2.0 ** -24)
    xyz, idx = dc.points_ref(coords, noise, ppc, C, H, float(bound))
    for cas in range(C):
        sl = slice(cas * ppc, (cas + 1) * ppc)
        bc = min(2 ** cas, bound)
        want = _torch_points(coords[sl], noise[sl], H, bc, literal=False)
        np.testing.assert_array_equal(xyz[sl].view(np.uint32), want.view(np.uint32))
        lit = _torch_points(coords[sl], noise[sl], H, bc, literal=True)
        if H <= 4:
            np.testing.assert_array_equal(xyz[sl].view(np.uint32), lit.view(np.uint32))
        else:
            assert np.abs(xyz[sl].astype(np.float64) - lit).max() <= 12 * 2.0 ** -24 * bc
        assert np.array_equal(idx[sl], cas * H ** 3 + oracle.morton3D(coords[sl]))


@pytest.mark.parametrize("H,C,bound", [(2, 1, 1.0), (4, 3, 3.0), (8, 2, 2.0)])
def test_points_ref_all_cell_mode_is_the_meshgrid_update(H, C, bound):
    """coords None = the reference's full update (:516-538): every cell once per
    cascade, its noise the cell's meshgrid row; here point i is the cell of
    Morton code i, so index = cascade * H^3 + i."""
    H3 = H ** 3
    rng = np.random.default_rng(H)
    noise = rng.random((C * H3, 3)).astype(F32)
    xyz, idx = dc.points_ref(None, noise, H3, C, H, bound)
    assert np.array_equal(idx, np.arange(C * H3))
    xs = np.arange(H, dtype=np.int32)
    mesh = np.stack(np.meshgrid(xs, xs, xs, indexing="ij"), -1).reshape(-1, 3)
    mx, mi = dc.points_ref(np.tile(mesh, (C, 1)), noise, H3, C, H, bound)
    np.testing.assert_array_equal(xyz[mi].view(np.uint32), mx.view(np.uint32))


@pytest.mark.parametrize("tag,bound,thresh", CASES)
def test_restatements_replay_the_reference_fixture(tag, bound, thresh):
    f = _fixture()
    H = int(f["H"])
    C = 1 + int(np.ceil(np.log2(bound)))
    H3 = H ** 3
    cen = np.array([0.15, -0.1, 0.05], F32) * F32(bound)
    for u in range(4):
        prev = f[f"{tag}_marked"] if u == 0 else f[f"{tag}_u{u - 1}_grid"]
        d = _draws(f, tag, u)
        if u >= 2:
            ppc, cs, ns = 2 * (H3 // 4), [], []
            for cas in range(C):
                cells, picks, noise = d[3 * cas:3 * cas + 3]
                occ = np.nonzero(prev[cas] > 0)[0].astype(np.int32)
                cs.append(np.concatenate([cells.astype(np.int32), oracle.morton3D_invert(occ[picks])]))
                ns.append(noise)
            coords = np.concatenate(cs)
        else:
            ppc, ns, coords = H3, d, None
        xyz, idx = dc.points_ref(coords, np.concatenate(ns), ppc, C, H, float(bound))
        sig = (F32(30.0) * np.exp(-((xyz - cen) ** 2).sum(-1) / F32(0.35 * bound * bound))).astype(F32)
        tmp = dc.run_max_ref(np.full(C * H3, -1.0, F32), sig, idx)
        r = dc.ema_pack_ref(prev, tmp, 0.95, float(thresh))
        ref = f[f"{tag}_u{u}_grid"]
        assert np.array_equal(r["grid"].reshape(ref.shape) < 0, ref < 0)
        np.testing.assert_allclose(r["grid"].reshape(ref.shape), ref, rtol=RTOL, atol=1e-30)
        md = float(f[f"{tag}_u{u}_mean_density"])
        assert abs(float(r["mean"]) - md) <= RTOL * md
        assert _bits_match(r["bits"], f[f"{tag}_u{u}_bitfield"], ref, min(md, thresh)), u
        assert np.all(r["tmp"] == -1)


def test_ema_pack_ref_threshold_is_pythons_min():
    """min(mean, density_thresh) is `density_thresh if density_thresh < mean
    else mean`: a NaN mean stays NaN (every bit clear, as upstream's packbits
    at a NaN threshold), where `mean < density_thresh ? mean : density_thresh`
    would give density_thresh and light the cells above it."""
    g = np.array([np.nan, 50.0, 3.0, 0.0, -1.0, 50.0, 50.0, 50.0], F32)
    r = dc.ema_pack_ref(g, np.full(8, -1.0, F32), 0.95, 10.0)
    assert math.isnan(r["sum"]) and np.isnan(r["mean"]) and np.isnan(r["thresh"])
    assert not r["bits"].any()
    assert math.isnan(min(float("nan"), 10.0)) and min(10.0, float("nan")) == 10.0
    assert np.array_equal(oracle.packbits(g, float("nan")), r["bits"])


def _ema_cases():
    for name in dc.EMA_NAMES:
        for H in dc.EMA_H:
            for C in dc.EMA_C:
                yield name, C, H, dc.ema_case(name, C, H)
    yield "big", dc.BIG_C, dc.BIG_H, dc.ema_big_case()


def test_ema_cases_meet_their_conditions():
    seen_g, seen_pairs = set(), set()
    assert float(dc.ROUNDS) * float(F32(dc.DECAY)) != float(dc.ROUNDS * F32(dc.DECAY))  # the product rounds
    assert 0 < float(dc.DENORMAL) < float(np.finfo(F32).tiny)
    assert float(F32(0.01)) != 0.01
    for name, C, H, c in _ema_cases():
        n = C * H ** 3
        g, t = c["grid"], c["tmp"]
        assert g.shape == t.shape == (n,) and g.dtype == t.dtype == F32
        r = dc.ema_pack_ref(g, t, c["decay"], c["thresh"])
        with np.errstate(invalid="ignore"):
            valid = (g >= 0) & (t >= 0)
            # the select in ema_pack_ref is np.maximum up to the sign of a zero
            np.testing.assert_array_equal(r["grid"][valid], np.maximum(g * F32(c["decay"]), t)[valid])
            assert np.array_equal(r["grid"][~valid].view(np.uint32), g[~valid].view(np.uint32))
            at = valid & (r["grid"] == r["thresh"])
        # whatever order the device adds in, the fp32 mean (so the threshold) is this one
        assert dc.mean_is_robust(r["sum"], n), (name, C, H)
        bits = np.unpackbits(r["bits"], bitorder="little")
        if name == "cross_nan":
            assert np.isnan(g).any() and math.isnan(r["sum"]) and not bits.any()
        elif name == "cross_inf":
            assert r["sum"] == math.inf and float(r["thresh"]) == c["thresh"]
        else:
            assert math.isfinite(r["sum"])
        if name.startswith("tie"):
            assert at.any() and not bits[at].any()     # cells equal to the threshold: strict >, bit clear
            assert bits.any() and not bits.all()
            assert float(r["thresh"]) == (2.0 if name == "tie_mean" else float(F32(0.01)))
        if name == "tie_thresh":
            above = r["grid"] == np.nextafter(F32(0.01), F32(1))
            assert above.any() and bits[above].all()
            keep = (g == F32(0.01)) & (t == -1)
            assert keep.any() and np.all(r["grid"][keep] == F32(0.01))  # tmp -1: no decay
        if name == "big":
            assert n == 2 * 1024 * 256 * 4 and float(r["thresh"]) == float(r["mean"])
            assert 0.2 < bits.mean() < 0.8
        if name.startswith("cross"):
            with np.errstate(invalid="ignore"):
                undecayed = (g > 0) & (t == -1)
            if undecayed.any():
                assert np.array_equal(r["grid"][undecayed].view(np.uint32), g[undecayed].view(np.uint32))
            for gv, tv in zip(g.view(np.uint32), t.view(np.uint32)):
                seen_pairs.add((name, int(gv), int(tv)))
            seen_g.update(int(v) for v in g.view(np.uint32))
    # the cross product is complete over the sizes: every grid value with every tmp kind
    for gv in dc.GRID_VALUES:
        for kind in dc.TMP_KINDS:
            key = ("cross_nan", int(F32(gv).view(np.uint32)), int(dc.tmp_value(gv, kind).view(np.uint32)))
            assert key in seen_pairs, (gv, kind)
    assert {int(v) for v in dc.GRID_VALUES.view(np.uint32)} <= seen_g


def test_draw_grids_meet_their_conditions():
    for H in dc.DRAW_H:
        for C in dc.DRAW_C:
            H3 = H ** 3
            g = dc.draw_grid("empty_cascade", C, H)
            e = dc.empty_cascade_of(C, H)
            with np.errstate(invalid="ignore"):
                n_occ = (g > 0).sum(1)
            assert n_occ[e] == 0 and all(n_occ[c] > 0 for c in range(C) if c != e)
            row = g[e]
            assert (np.isnan(row).any() and (row == -1).any() and ((row == 0) & np.signbit(row)).any()
                    and ((row == 0) & ~np.signbit(row)).any())
            g = dc.draw_grid("first_cell", C, H)
            assert all(np.array_equal(np.nonzero(g[c] > 0)[0], [0]) for c in range(C))
            g = dc.draw_grid("last_cell", C, H)
            assert all(np.array_equal(np.nonzero(g[c] > 0)[0], [H3 - 1]) for c in range(C))
            assert (dc.draw_grid("full", C, H) > 0).all()
    g = dc.carry_grid()
    occ = np.nonzero(g[1] > 0)[0]
    assert not (g[0] > 0).any() and occ.min() == 1024 * 1024 and occ.max() == dc.CARRY_H ** 3 - 1
    blocks = np.unique(occ // 1024)
    assert blocks.min() == 1024 and blocks.size > 512  # counts in the scan's second stride of 1024 blocks


def test_run_max_cases_meet_their_conditions():
    for pattern in dc.RUN_PATTERNS:
        for H in dc.RUN_H:
            for C in dc.RUN_C:
                H3, N = H ** 3, H ** 3 // 4
                idx, sigma, tmp = dc.run_max_case(pattern, C, H)
                assert idx.shape == sigma.shape == (C * 2 * N,) and tmp.shape == (C * H3,)
                cas = np.repeat(np.arange(C), 2 * N)
                assert np.all((idx >= cas * H3) & (idx < (cas + 1) * H3))  # every index inside its cascade
                halves = idx.reshape(2 * C, N)
                assert np.all(np.diff(halves, axis=1) >= 0)  # sorted within each half, as the draws are
                want = dc.run_max_ref(tmp, sigma, idx)
                drawn = np.zeros(C * H3, bool)
                drawn[idx] = True
                assert np.array_equal(want[~drawn], tmp[~drawn])
                kept = drawn & (want == tmp) & (tmp == dc.TMP_PALETTE[2])
                raised = drawn & (want > tmp)
                assert kept.any() and raised.any()  # a scratch value above its cell's densities is kept
                if pattern == "single":
                    assert all(np.unique(halves[2 * c + 1]).size == 1 for c in range(C))
                if pattern == "distinct":
                    assert np.unique(idx).size == idx.size
                if pattern == "both_halves":
                    X = H3 // 2
                    assert all((halves[2 * c] == c * H3 + X).sum() >= 3 and (halves[2 * c + 1] == c * H3 + X).sum() >= 4
                               for c in range(C))
                if pattern == "boundary":
                    assert all(halves[2 * c][-1] == halves[2 * c][-3] == halves[2 * c + 1][0] == halves[2 * c + 1][1]
                               for c in range(C))
    for v in (0.0, 1e-40, 1e30, np.inf):
        assert F32(v) in dc.SIGMA_PALETTE
    assert np.unique(dc.SIGMA_PALETTE).size < dc.SIGMA_PALETTE.size  # ties
    # the cut runs: a slice boundary strictly inside a run of >= 3 equal indices
    pattern, C, H = dc.SPLIT_CASE
    idx = dc.run_max_case(pattern, C, H)[0]
    N = H ** 3 // 4
    assert max(dc.run_length_at(idx, N, s) for s in range(idx.size + 1)) >= 3
    pattern, C, H = dc.THREE_WAY_CASE
    idx = dc.run_max_case(pattern, C, H)[0]
    s1, s2 = dc.three_way_cuts(idx, H ** 3 // 4)
    assert dc.run_length_at(idx, H ** 3 // 4, s1) >= 3 and len({s1, s2 - s1, idx.size - s2}) == 3
    pattern, C, H, lo, hi = dc.LONG_SLICE
    assert hi - lo > 256 and (hi - lo) % 256 and hi <= C * 2 * (H ** 3 // 4)


def test_draws_take_the_uniform_cells_where_a_cascade_is_empty():
    """The restated draws on an empty cascade: the occupied half falls back to
    uniform cells (upstream's randint(0, 0) cannot draw at all), and on a
    single occupied cell every draw of the occupied half is that cell."""
    C, H = 2, 8
    H3, N = H ** 3, H ** 3 // 4
    g = dc.draw_grid("empty_cascade", C, H)
    e = dc.empty_cascade_of(C, H)
    coords, _ = dc._draws(3, 17, C * 2 * N, 2 * N, H, g)
    cells = oracle.morton3D(coords).reshape(C, 2, N)
    assert np.unique(cells[e, 1]).size > N // 4            # spread over the cube, not one cell
    assert np.all(g[1 - e][cells[1 - e, 1]] > 0)
    cells = dc._draws_ostat(3, 17, C, H, g)[2].reshape(C, 2, N)
    assert np.unique(cells[e, 1]).size > N // 4 and np.all(g[1 - e][cells[1 - e, 1]] > 0)
    for kind, cell in (("first_cell", 0), ("last_cell", H3 - 1)):
        g = dc.draw_grid(kind, C, H)
        assert np.all(dc._draws_ostat(3, 17, C, H, g)[2].reshape(C, 2, N)[:, 1] == cell)
        assert np.all(oracle.morton3D(dc._draws(3, 17, C * 2 * N, 2 * N, H, g)[0]).reshape(C, 2, N)[:, 1] == cell)


def test_renderer_rejects_a_grid_size_that_is_no_power_of_two():
    from nerf.renderer import NeRFRenderer
    for bad in (6, 100, 0, 1, 2048):
        with pytest.raises(ValueError, match="grid_size"):
            NeRFRenderer(grid_size=bad)
    assert NeRFRenderer(grid_size=16, cuda_ray=True).density_grid.shape == (1, 16 ** 3)
