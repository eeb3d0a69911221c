"""GPU: every entry of the density-grid update (csrc/density_grid.hip) called
through _ngp_native on made-up buffers, at small grids and edge values,
against the numpy restatements of tests/density_cases.py (proved on the CPU by
tests/test_density_cases_cpu.py). Every output buffer starts as a sentinel
with a guard behind it and nothing outside the expected range may change;
everything is compared bit for bit, but for the EMA's sum: stats[0] within
n * 2^-53 relative of math.fsum (the worst case of n non-negative fp64 terms
added in any order).

  run_max       every index pattern x H x C; every two-way split of one case, a
                three-way split, a slice of 600; empty slice; argument errors
  draw          draw order: cells and noise = _draws; full mode leaves coords
  draw_sorted   Morton order: indices = _draws_ostat, xyz = points_ref; slices
                inside a half; on grids with an empty cascade, one occupied cell
                (first / last), every cell occupied, and the scan's carry
  points        all-cell and coords mode at H 2, 4, C 1, 3, 16, four bounds
  points_sorted one bucket per cascade; a tile, a tile + 1, a slice from 16383
  ema_pack      grid x tmp value cross product, threshold ties, NaN, two passes
  trainer       density_run_max=True and False give the same grid and bitfield
"""
import copy
import math

import numpy as np
import pytest
import torch

import density_cases as dc

pytestmark = pytest.mark.gpu

F32 = np.float32
ERR_ARG = -1  # NGP_ERR_ARG
GUARD = 64
SENT_F, SENT_I, SENT_D = -777.25, -77777777, -5.0
BOUNDS = (1.0, 2.0, 3.0)  # by C - 1: the last cascade of C = 3 is cut at bound 3 < 2^2


@pytest.fixture(scope="module")
def nat(cuda):
    import _ngp_native as nat
    nat.lib()
    return nat


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _sent(shape, dtype, cuda):
    """A sentinel-filled buffer of `shape` plus GUARD rows."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    fill = {torch.float32: SENT_F, torch.int32: SENT_I, torch.float64: SENT_D, torch.uint8: 0xA5}[dtype]
    return torch.full((shape[0] + GUARD,) + shape[1:], fill, dtype=dtype, device=cuda)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want):
    np.testing.assert_array_equal(_bits(got), _bits(want))


def _untouched(buf, start):
    """Rows [start:] of a _sent buffer still hold the sentinel."""
    tail = buf[start:]
    fill = {torch.float32: SENT_F, torch.int32: SENT_I, torch.float64: SENT_D, torch.uint8: 0xA5}[buf.dtype]
    assert bool((tail == fill).all()), "written outside the expected range"


# ---- ngp_density_grid_run_max ---------------------------------------------------------------

class _RunMax:
    """One case on the device. A slice [lo, hi) is copied to the head of fresh
    sigma / index buffers (as the trainer holds it), with a guard on both sides
    that would change the result if read: the neighbouring index repeated, with
    an infinite density."""

    def __init__(self, nat, cuda, pattern, C, H):
        self.nat, self.cuda, self.C, self.H = nat, cuda, C, H
        self.idx, self.sigma, self.tmp = dc.run_max_case(pattern, C, H)
        self.P = self.idx.size

    def fresh_tmp(self, rows=1):
        t = _sent((rows, self.tmp.size + GUARD), torch.float32, self.cuda)[:rows]
        t[:, :self.tmp.size] = _dev(self.tmp, self.cuda)
        return t

    def fold(self, tmp_row, lo, hi):
        n = hi - lo
        idx = np.empty(n + 2 * GUARD, np.int32)
        sig = np.full(n + 2 * GUARD, np.inf, F32)
        idx[GUARD:GUARD + n], sig[GUARD:GUARD + n] = self.idx[lo:hi], self.sigma[lo:hi]
        idx[:GUARD] = self.idx[lo] if n else 0
        idx[GUARD + n:] = self.idx[hi - 1] if n else 0
        ti, ts = _dev(idx, self.cuda), _dev(sig, self.cuda)
        rc = self.nat.lib().ngp_density_grid_run_max(ts.data_ptr() + 4 * GUARD, ti.data_ptr() + 4 * GUARD, self.C,
                                                     self.H, lo, hi, tmp_row.data_ptr(), self.nat.stream_of(ts))
        torch.cuda.synchronize()  # ti / ts stay alive until the launch is done
        return rc

    def want(self, lo=0, hi=None):
        return dc.run_max_ref(self.tmp, self.sigma[lo:hi], self.idx[lo:hi])


def _check_tmp(case, tmp_row, want):
    _same(tmp_row[:want.size], want)
    _untouched(tmp_row, want.size)


@pytest.mark.parametrize("pattern", dc.RUN_PATTERNS)
def test_run_max_whole_range(nat, cuda, pattern):
    for H in dc.RUN_H:
        for C in dc.RUN_C:
            case = _RunMax(nat, cuda, pattern, C, H)
            t = case.fresh_tmp()
            nat.check(case.fold(t[0], 0, case.P), "run_max")
            _check_tmp(case, t[0], case.want())


def test_run_max_every_two_way_split(nat, cuda):
    """[0, s) then [s, P) into one tmp, for every s: a run cut by the slice
    boundary has its maximum taken in two parts, a run ending at a half
    boundary stops there, and the union is the whole range's result."""
    pattern, C, H = dc.SPLIT_CASE
    case = _RunMax(nat, cuda, pattern, C, H)
    t = case.fresh_tmp(rows=case.P + 1)
    for s in range(case.P + 1):
        nat.check(case.fold(t[s], 0, s), "run_max")
        if s in (1, case.P // 2, case.P - 1):  # one slice alone: only its own points
            _check_tmp(case, t[s], case.want(0, s))
        nat.check(case.fold(t[s], s, case.P), "run_max")
    want = case.want()
    for s in range(case.P + 1):
        _check_tmp(case, t[s], want)


def test_run_max_three_way_split_and_a_long_slice(nat, cuda):
    pattern, C, H = dc.THREE_WAY_CASE
    case = _RunMax(nat, cuda, pattern, C, H)
    s1, s2 = dc.three_way_cuts(case.idx, H ** 3 // 4)
    t = case.fresh_tmp()
    for lo, hi in ((s2, case.P), (0, s1), (s1, s2)):  # any order: the fold is a max
        nat.check(case.fold(t[0], lo, hi), "run_max")
    _check_tmp(case, t[0], case.want())
    pattern, C, H, lo, hi = dc.LONG_SLICE
    case = _RunMax(nat, cuda, pattern, C, H)
    t = case.fresh_tmp()
    nat.check(case.fold(t[0], lo, hi), "run_max")
    _check_tmp(case, t[0], case.want(lo, hi))


def test_run_max_empty_slice_and_argument_errors(nat, cuda):
    case = _RunMax(nat, cuda, "ostat", 2, 4)
    lib, P = nat.lib(), case.P
    t = case.fresh_tmp()
    for lo in (0, 7, P):
        nat.check(case.fold(t[0], lo, lo), "run_max")
    _check_tmp(case, t[0], case.tmp)
    sig, idx = _dev(case.sigma, cuda), _dev(case.idx, cuda)
    s = nat.stream_of(sig)

    def call(sigma=sig, indices=idx, C=2, H=4, lo=0, hi=P, tmp=t):
        return lib.ngp_density_grid_run_max(nat.ptr(sigma), nat.ptr(indices), C, H, lo, hi, nat.ptr(tmp), s)

    assert call(sigma=None) == ERR_ARG and call(indices=None) == ERR_ARG and call(tmp=None) == ERR_ARG
    assert call(lo=5, hi=4) == ERR_ARG
    assert call(hi=P + 1) == ERR_ARG
    assert call(H=1) == ERR_ARG and call(H=0) == ERR_ARG
    assert call(H=3) == ERR_ARG and call(H=6) == ERR_ARG and call(H=2048) == ERR_ARG
    assert call(C=0) == ERR_ARG and call(C=17, hi=0) == ERR_ARG
    assert call(C=16, H=1024, hi=0) == ERR_ARG  # 2^34 cells: not countable in 32 bits
    torch.cuda.synchronize()
    _check_tmp(case, t[0], case.tmp)  # nothing was launched


# ---- ngp_density_grid_draw / ngp_density_grid_draw_sorted ------------------------------------

def _draw_ws(nat, cuda, C, H):
    lib = nat.lib()
    dws = torch.zeros(int(lib.ngp_density_grid_draw_workspace_bytes(C, H)), dtype=torch.uint8, device=cuda)
    ows = torch.zeros(int(lib.ngp_density_grid_ostat_workspace_bytes(C, H)), dtype=torch.uint8, device=cuda)
    return dws, ows


def _check_draw(nat, cuda, grid, C, H, seed, update):
    """ngp_density_grid_draw, partial and full, against _draws."""
    lib, P_ = nat.lib(), nat.ptr
    H3, N = H ** 3, H ** 3 // 4
    g = _dev(grid, cuda)
    dws, _ = _draw_ws(nat, cuda, C, H)
    s = nat.stream_of(g)
    P = C * 2 * N
    coords, noise = _sent((P, 3), torch.int32, cuda), _sent((P, 3), torch.float32, cuda)
    nat.check(lib.ngp_density_grid_draw(P_(g), C, H, 1, seed, update, P_(coords), P_(noise), P_(dws), dws.numel(), s),
              "draw")
    torch.cuda.synchronize()
    wc, wn = dc._draws(seed, update, P, 2 * N, H, grid)
    _same(coords[:P], wc)
    _same(noise[:P], wn)
    _untouched(coords, P)
    _untouched(noise, P)
    # full mode: the noise of every cell; coords (and the grid, the workspace) unused
    P = C * H3
    coords, noise = _sent((P, 3), torch.int32, cuda), _sent((P, 3), torch.float32, cuda)
    nat.check(lib.ngp_density_grid_draw(None, C, H, 0, seed, update, P_(coords), P_(noise), None, 0, s), "draw")
    torch.cuda.synchronize()
    _same(noise[:P], dc._draws(seed, update, P, H3, H)[1])
    _untouched(noise, P)
    _untouched(coords, 0)


def _check_draw_sorted(nat, cuda, grid, C, H, seed, update, bound, slices):
    """ngp_density_grid_draw_sorted over each [lo, hi) against _draws_ostat's
    cells and points_ref's arithmetic on them."""
    lib, P_ = nat.lib(), nat.ptr
    H3, N = H ** 3, H ** 3 // 4
    P = C * 2 * N
    g = _dev(grid, cuda)
    dws, ows = _draw_ws(nat, cuda, C, H)
    s = nat.stream_of(g)
    coords, noise, cells = dc._draws_ostat(seed, update, C, H, grid)
    want_idx = (np.repeat(np.arange(C), 2 * N) * H3 + cells).astype(np.int32)
    want_xyz, pidx = dc.points_ref(coords, noise, 2 * N, C, H, bound)
    assert np.array_equal(pidx, want_idx)
    for lo, hi in slices(P, N):
        xyz, idx = _sent((hi - lo, 3), torch.float32, cuda), _sent(hi - lo, torch.int32, cuda)
        nat.check(lib.ngp_density_grid_draw_sorted(P_(g), C, H, seed, update, bound, lo, hi, P_(dws), dws.numel(),
                                                   P_(ows), ows.numel(), P_(xyz), P_(idx), s), "draw_sorted")
        torch.cuda.synchronize()
        _same(idx[:hi - lo], want_idx[lo:hi])
        _same(xyz[:hi - lo], want_xyz[lo:hi])
        _untouched(xyz, hi - lo)
        _untouched(idx, hi - lo)
    return cells


def _slices(P, N):
    """The whole range; a slice inside the first uniform half; one inside the
    last occupied half; two empty ones."""
    return [(0, P), (N // 2 + 1, N - 1), (P - N + 1, P - 2), (0, 0), (P - N + 3, P - N + 3)]


@pytest.mark.parametrize("kind", dc.DRAW_KINDS)
def test_draw_matches_restatement(nat, cuda, kind):
    for H in dc.DRAW_H:
        for C in dc.DRAW_C:
            _check_draw(nat, cuda, dc.draw_grid(kind, C, H), C, H, seed=21 + H, update=16 + C)


@pytest.mark.parametrize("kind", dc.DRAW_KINDS)
def test_draw_sorted_matches_restatement(nat, cuda, kind):
    for H in dc.DRAW_H:
        for C in dc.DRAW_C:
            grid = dc.draw_grid(kind, C, H)
            cells = _check_draw_sorted(nat, cuda, grid, C, H, 21 + H, 16 + C, BOUNDS[C - 1], _slices)
            N = H ** 3 // 4
            occ_half = cells.reshape(C, 2, N)[:, 1]
            if kind == "first_cell":
                assert np.all(occ_half == 0)
            if kind == "last_cell":
                assert np.all(occ_half == H ** 3 - 1)
            if kind == "empty_cascade":  # the empty cascade's occupied half: uniform cells
                assert np.unique(occ_half[dc.empty_cascade_of(C, H)]).size > min(N, 64) // 4


def test_draws_on_the_grid_that_needs_the_scan_carry(nat, cuda):
    """H = 128, C = 2, occupied cells only in cascade 1's blocks >= 1024: their
    offsets in the occupied list come from the scan's second stride."""
    grid = dc.carry_grid()
    C, H = dc.CARRY_C, dc.CARRY_H
    N = H ** 3 // 4
    cells = _check_draw_sorted(nat, cuda, grid, C, H, 5, 16, 2.0, lambda P, N: [(0, P)])
    assert np.all(cells.reshape(C, 2, N)[1, 1] >= 1024 * 1024)
    lib, P_ = nat.lib(), nat.ptr
    g = _dev(grid, cuda)
    dws, _ = _draw_ws(nat, cuda, C, H)
    P = C * 2 * N
    coords, noise = _sent((P, 3), torch.int32, cuda), _sent((P, 3), torch.float32, cuda)
    nat.check(lib.ngp_density_grid_draw(P_(g), C, H, 1, 5, 16, P_(coords), P_(noise), P_(dws), dws.numel(),
                                        nat.stream_of(g)), "draw")
    torch.cuda.synchronize()
    wc, wn = dc._draws(5, 16, P, 2 * N, H, grid)
    _same(coords[:P], wc)
    _same(noise[:P], wn)
    _untouched(coords, P)


def test_draw_argument_errors(nat, cuda):
    lib, P_ = nat.lib(), nat.ptr
    C, H = 2, 4
    g = _dev(dc.draw_grid("full", 3, 8), cuda)  # room for every shape tried below
    dws, ows = _draw_ws(nat, cuda, 3, 8)
    coords, noise = _sent((4096, 3), torch.int32, cuda), _sent((4096, 3), torch.float32, cuda)
    xyz, idx = _sent((4096, 3), torch.float32, cuda), _sent(4096, torch.int32, cuda)
    s = nat.stream_of(g)

    def draw(C=C, H=H, partial=1, grid=g, co=coords, no=noise, ws=dws, wsb=None):
        return lib.ngp_density_grid_draw(P_(grid), C, H, partial, 1, 16, P_(co), P_(no), P_(ws),
                                         dws.numel() if wsb is None else wsb, s)

    def draw_sorted(C=C, H=H, lo=0, hi=0, grid=g, x=xyz):
        return lib.ngp_density_grid_draw_sorted(P_(grid), C, H, 1, 16, 1.0, lo, hi, P_(dws), dws.numel(), P_(ows),
                                                ows.numel(), P_(x), P_(idx), s)

    for f in (draw, draw_sorted):
        for bad in (dict(H=1), dict(H=3), dict(H=6), dict(H=2048), dict(C=0), dict(C=17), dict(C=16, H=1024)):
            assert f(**bad) == ERR_ARG, (f.__name__, bad)
        assert b"power of two" in lib.ngp_last_error()
        assert f(grid=None) == ERR_ARG
    for partial in (0, 1):
        assert draw(partial=partial, H=6) == ERR_ARG and draw(partial=partial, no=None) == ERR_ARG
    assert draw(co=None) == ERR_ARG and draw(ws=None) == ERR_ARG and draw(wsb=16) == ERR_ARG
    P = C * 2 * (H ** 3 // 4)
    assert draw_sorted(lo=3, hi=2) == ERR_ARG and draw_sorted(hi=P + 1) == ERR_ARG and draw_sorted(x=None) == ERR_ARG
    torch.cuda.synchronize()
    for buf in (coords, noise, xyz, idx):
        _untouched(buf, 0)


# ---- ngp_density_grid_points / ngp_density_grid_points_sorted --------------------------------

POINT_H, POINT_C, POINT_BOUNDS = (2, 4), (1, 3, 16), (1.0, 2.0, 3.0, 16.0)


def _coords_case(C, H, ppc, seed):
    rng = np.random.default_rng(seed)
    coords = rng.integers(0, H, (C * ppc, 3)).astype(np.int32)
    coords[0], coords[-1] = 0, H - 1  # the cube's two extreme cells
    noise = rng.random((C * ppc, 3)).astype(F32)
    noise[0], noise[-1] = 0.0, F32(1 - 2.0 ** -24)
    return coords, noise


def test_points_all_cell_and_coords_modes(nat, cuda):
    lib, P_ = nat.lib(), nat.ptr
    for H in POINT_H:
        for C in POINT_C:
            for bound in POINT_BOUNDS:
                H3 = H ** 3
                for ppc, coords in ((H3, None), (37, True)):  # C = 16: 592 points, three blocks
                    P = C * ppc
                    if coords is None:
                        noise = np.random.default_rng(H + C).random((P, 3)).astype(F32)
                    else:
                        coords, noise = _coords_case(C, H, ppc, 100 * H + C)
                    tn = _dev(noise, cuda)
                    tc = None if coords is None else _dev(coords, cuda)
                    xyz, idx = _sent((P, 3), torch.float32, cuda), _sent(P, torch.int32, cuda)
                    nat.check(lib.ngp_density_grid_points(P_(tc), P_(tn), P, ppc, C, H, bound, P_(xyz), P_(idx),
                                                          nat.stream_of(tn)), "points")
                    torch.cuda.synchronize()
                    wx, wi = dc.points_ref(coords, noise, ppc, C, H, bound)
                    _same(xyz[:P], wx)
                    _same(idx[:P], wi)
                    _untouched(xyz, P)
                    _untouched(idx, P)
                    assert wi.min() >= 0 and wi.max() < C * H3
                    if coords is None:
                        assert np.array_equal(wi, np.arange(P))  # point i of a cascade is cell i


@pytest.mark.parametrize("H", [2, 4, 16, 128])
def test_points_ref_is_the_reference_expression_on_the_device(cuda, H):
    """The reference's own expressions (renderer.py:524, :528-533), literally,
    in torch on the device, where upstream runs them: points_ref bit for bit at
    every H and bound. (On the CPU torch divides `/ (H - 1)` truly and the
    literal form is an ulp off at H = 16 and 128: test_density_cases_cpu.py.)"""
    for bound in (1, 2, 3, 16):
        C = 1 + math.ceil(math.log2(bound))
        rng = np.random.default_rng(100 * H + bound)
        ppc = 4096
        coords = rng.integers(0, H, (C * ppc, 3)).astype(np.int32)
        coords[:H] = np.arange(H, dtype=np.int32)[:, None]
        noise = rng.random((C * ppc, 3)).astype(F32)
        want, _ = dc.points_ref(coords, noise, ppc, C, H, float(bound))
        tc, tn = _dev(coords, cuda), _dev(noise, cuda)
        for cas in range(C):
            sl = slice(cas * ppc, (cas + 1) * ppc)
            xyzs = 2 * tc[sl].float() / (H - 1) - 1
            bc = min(2 ** cas, bound)
            hgs = bc / H
            cas_xyzs = xyzs * (bc - hgs)
            cas_xyzs += (tn[sl] * 2 - 1) * hgs
            _same(cas_xyzs, want[sl])


def _bucket(idx, C, H):
    """ngp_density_grid_points_sorted's brick: (cascade, morton >> shift), with
    bricks of >= 2^9 cells and at most 8192 buckets over the cascades."""
    H3 = H ** 3
    bits = int(np.ceil(np.log2(H)))
    shift = min(9, 3 * bits)
    while shift < 3 * bits and C << (3 * bits - shift) > 8192:
        shift += 1
    idx = idx.astype(np.int64)
    return (idx // H3) * (1 << (3 * bits - shift)) + ((idx % H3) >> shift), 1 << (3 * bits - shift)


def _rows(xyz, idx):
    r = np.concatenate([_bits(xyz).astype(np.int64), np.asarray(idx, np.int64)[:, None]], 1)
    return r[np.lexsort(r.T[::-1])]  # rows as a sorted multiset


def _check_sorted(nat, cuda, C, H, ppc, bound, slices, seed):
    lib, P_ = nat.lib(), nat.ptr
    P = C * ppc
    coords, noise = _coords_case(C, H, ppc, seed)
    tc, tn = _dev(coords, cuda), _dev(noise, cuda)
    wx, wi = dc.points_ref(coords, noise, ppc, C, H, bound)
    ws = torch.full((int(lib.ngp_density_grid_sort_workspace_bytes(C, H)),), 0xA5, dtype=torch.uint8, device=cuda)
    for lo, hi in slices:
        n = hi - lo
        xyz, idx = _sent((n, 3), torch.float32, cuda), _sent(n, torch.int32, cuda)
        nat.check(lib.ngp_density_grid_points_sorted(P_(tc), P_(tn), P, ppc, C, H, bound, lo, hi, P_(ws), ws.numel(),
                                                     P_(xyz), P_(idx), nat.stream_of(tc)), "points_sorted")
        torch.cuda.synchronize()
        _untouched(xyz, n)
        _untouched(idx, n)
        gi = idx[:n].cpu().numpy()
        np.testing.assert_array_equal(_rows(xyz[:n], gi), _rows(wx[lo:hi], wi[lo:hi]))
        b, nb = _bucket(gi, C, H)
        assert np.all(np.diff(b) >= 0)
    return nb


def test_points_sorted_one_bucket_per_cascade(nat, cuda):
    """H = 2 and 4: a cascade is one brick, so the order is the cascades';
    slices that begin and end inside cascade 1, an empty one, the whole."""
    for H in POINT_H:
        for C in (2, 3, 16):
            ppc = 2 * (H ** 3 // 4)
            P = C * ppc
            slices = [(0, P), (ppc + 1, 2 * ppc - 1), (ppc + ppc // 2, ppc + ppc // 2 + 1), (ppc, ppc), (1, P - 1)]
            assert _check_sorted(nat, cuda, C, H, ppc, BOUNDS[min(C, 3) - 1], slices, 7 * H + C) == 1


def test_points_sorted_tile_edges(nat, cuda):
    """H = 32, C = 2 (64 bricks a cascade): slices of exactly one 16384-point
    tile, of a tile and one point, and from one point before the second
    cascade to the end."""
    C, H = 2, 32
    ppc = H ** 3 // 2
    assert ppc == 16384
    nb = _check_sorted(nat, cuda, C, H, ppc, 2.0, [(0, 16384), (0, 16385), (16383, 32768)], 3)
    assert nb == 64


def test_points_argument_errors(nat, cuda):
    lib, P_ = nat.lib(), nat.ptr
    C, H, ppc = 2, 4, 32
    coords, noise = _coords_case(3, 8, 512, 1)  # room for every shape tried below
    tc, tn = _dev(coords, cuda), _dev(noise, cuda)
    xyz, idx = _sent((4096, 3), torch.float32, cuda), _sent(4096, torch.int32, cuda)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    s = nat.stream_of(tc)

    def points(C=C, H=H, ppc=ppc, P=None, co=tc, no=tn, x=xyz):
        return lib.ngp_density_grid_points(P_(co), P_(no), C * ppc if P is None else P, ppc, C, H, 1.0, P_(x),
                                           P_(idx), s)

    def points_sorted(C=C, H=H, ppc=ppc, P=None, lo=0, hi=0, co=tc, no=tn, x=xyz, w=ws, wb=None):
        return lib.ngp_density_grid_points_sorted(P_(co), P_(no), C * ppc if P is None else P, ppc, C, H, 1.0, lo, hi,
                                                  P_(w), ws.numel() if wb is None else wb, P_(x), P_(idx), s)

    for f in (points, points_sorted):
        for bad in (dict(H=1), dict(H=3), dict(H=6), dict(H=2048), dict(C=0), dict(C=17), dict(C=16, H=1024)):
            assert f(**bad) == ERR_ARG, (f.__name__, bad)
        assert b"power of two" in lib.ngp_last_error()
        assert f(no=None) == ERR_ARG and f(x=None) == ERR_ARG
        assert f(P=C * ppc + 1) == ERR_ARG and f(ppc=0, P=0) == ERR_ARG
    assert points(co=None, ppc=32) == ERR_ARG  # all-cell mode needs ppc = H^3
    assert points_sorted(co=None) == ERR_ARG and points_sorted(w=None) == ERR_ARG and points_sorted(wb=0) == ERR_ARG
    assert points_sorted(lo=2, hi=1) == ERR_ARG and points_sorted(hi=C * ppc + 1) == ERR_ARG
    torch.cuda.synchronize()
    _untouched(xyz, 0)
    _untouched(idx, 0)


# ---- ngp_density_grid_ema_pack ----------------------------------------------------------------

def _check_ema(nat, cuda, case, C, H, thresh=None):
    lib, P_ = nat.lib(), nat.ptr
    n = C * H ** 3
    thresh = case["thresh"] if thresh is None else thresh
    want = dc.ema_pack_ref(case["grid"], case["tmp"], case["decay"], thresh)
    grid, tmp = _sent(n, torch.float32, cuda), _sent(n, torch.float32, cuda)
    grid[:n], tmp[:n] = _dev(case["grid"], cuda), _dev(case["tmp"], cuda)
    bits = _sent(n // 8, torch.uint8, cuda)
    stats = _sent(nat.DENSITY_STATS_LEN, torch.float64, cuda)
    nat.check(lib.ngp_density_grid_ema_pack(P_(grid), P_(tmp), C, H, case["decay"], thresh, P_(stats), P_(bits),
                                            nat.stream_of(grid)), "ema_pack")
    torch.cuda.synchronize()
    _same(grid[:n], want["grid"])
    _same(tmp[:n], want["tmp"])
    _same(bits[:n // 8], want["bits"])
    for buf, end in ((grid, n), (tmp, n), (bits, n // 8), (stats, 1 + min(-(-n // 256), 1024))):
        _untouched(buf, end)
    got = float(stats[0].item())
    print(f"ema_pack n={n} sum={got!r} fsum={want['sum']!r}")
    if math.isfinite(want["sum"]):
        assert abs(got - want["sum"]) <= dc.sum_bound(n) * want["sum"]
    else:
        assert math.isnan(got) == math.isnan(want["sum"]) and math.isinf(got) == math.isinf(want["sum"])
        assert math.isnan(got) or got > 0
    return want


@pytest.mark.parametrize("name", dc.EMA_NAMES)
def test_ema_pack_cases(nat, cuda, name):
    for H in dc.EMA_H:
        for C in dc.EMA_C:
            want = _check_ema(nat, cuda, dc.ema_case(name, C, H), C, H)
            if name == "cross_nan":
                assert not want["bits"].any()


def test_ema_pack_nan_density_thresh_takes_the_mean(nat, cuda):
    """min(mean, nan) is the mean in Python (nan < mean is False)."""
    want = _check_ema(nat, cuda, dc.ema_case("tie_mean", 2, 4), 2, 4, thresh=float("nan"))
    assert float(want["thresh"]) == 2.0 and want["bits"].any()


def test_ema_pack_two_passes(nat, cuda):
    want = _check_ema(nat, cuda, dc.ema_big_case(), dc.BIG_C, dc.BIG_H)
    assert float(want["thresh"]) == float(want["mean"])


def test_ema_pack_argument_errors(nat, cuda):
    lib, P_ = nat.lib(), nat.ptr
    n = 3 * 8 ** 3  # room for every shape tried below
    grid, tmp = _sent(n, torch.float32, cuda), _sent(n, torch.float32, cuda)
    bits, stats = _sent(n // 8, torch.uint8, cuda), _sent(nat.DENSITY_STATS_LEN, torch.float64, cuda)
    s = nat.stream_of(grid)

    def call(C=2, H=4, g=grid, t=tmp, st=stats, b=bits):
        return lib.ngp_density_grid_ema_pack(P_(g), P_(t), C, H, 0.95, 0.01, P_(st), P_(b), s)

    for bad in (dict(H=1), dict(H=3), dict(H=6), dict(H=2048), dict(C=0), dict(C=17), dict(C=16, H=1024),
                dict(g=None), dict(t=None), dict(st=None), dict(b=None)):
        assert call(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    for buf in (grid, tmp, bits, stats):
        _untouched(buf, 0)


# ---- the trainer's two routes from densities to tmp_grid --------------------------------------

def test_trainer_run_max_route_gives_the_same_grid(cuda):
    """FusedTrainer with density_run_max=True (densities per point, then
    ngp_density_grid_run_max) and False (the MLP epilogue's atomic max): after
    2 full and 3 partial updates the grid, bitfield and mean are identical."""
    from nerf.fused import FusedTrainer
    from nerf.provider import SyntheticLego
    from test_gpu_density import _model
    a = _model(cuda, bound=2)
    b = copy.deepcopy(a)
    fa = FusedTrainer(a, SyntheticLego(cuda, num_rays=256), M=20000, seed=5, options=dict(density_run_max=True))
    fb = FusedTrainer(b, SyntheticLego(cuda, num_rays=256), M=20000, seed=5, options=dict(density_run_max=False))
    assert fa.options["density_run_max"] and not fb.options["density_run_max"]
    for it in range(5):
        if it == 2:
            a.iter_density = b.iter_density = 16  # partial updates from here on
        fa.update_density()
        fb.update_density()
        torch.cuda.synchronize()
        _same(a.density_grid, b.density_grid.cpu().numpy())
        assert torch.equal(a.density_bitfield, b.density_bitfield)
        assert fa.mean_density == fb.mean_density and fa.mean_density > 0
    bits = np.unpackbits(a.density_bitfield.cpu().numpy())
    assert 0 < bits.sum() < bits.size
