"""The exact-sum grid cases (tests/grid_cases.py) are what they claim: the
conditions that make a ZERO tolerance legitimate on the device, checked on
the CPU oracle for every case before any device run.

1. every output grad of every row is nonzero (the binned backward drops
   all-zero rows, so zero padding would produce no items);
2. the float64 scatter of the live rows (times the accumulating calls) is its
   own round trip through the table's type: the expected table is exact;
3. enough entries of the hashed levels expect a nonzero value, so an all-zero
   or a mostly-untouched table cannot pass (1000 for the fused cases; the
   generic cases' tables and lattices are smaller, their floors are in the
   case table);
4. where terms are added one by one in fp16 (the fused backward's levels past
   the binned prefix, the generic fp16 kernel) the sum of |terms| of every
   entry is below 4: every term is a multiple of 2^-9, so every partial sum in
   any order is a multiple of 2^-9 below 4, an fp16 number;
5. on the binned levels, any window of consecutive live rows in one cell (what
   an in-wave run merge adds up before its single rounding to half) sums to
   less than 4 in |value|, again an fp16 number; the exact integer sum of the
   runs then rounds once, to the value of condition 2.
"""
import numpy as np
import pytest

import grid_cases as gc
import oracle


@pytest.mark.parametrize("name", list(gc.EXACT))
def test_exact_case_conditions(name):
    case = gc.EXACT[name]
    d = gc.exact_data(name)
    x, g, pid, ref, mag, offs = d["x"], d["g"], d["pid"], d["ref"], d["mag"], d["offs"]
    n, L, C = case.n, case.L, case.C
    # the level scales are odd integers and the rows are on the lattice
    for l in range(L):
        s, _ = gc.level_scale(l, case.scale, case.H)
        assert s == int(s) and int(s) % 2 == 1 and s < 2 ** 22, (l, s)
    q = x[pid >= 0] * (case.nlat - 1)
    assert np.array_equal(q, np.round(q)) and q.min() >= 0 and q.max() <= case.nlat - 1
    assert (pid[list(case.oob)] == -1).all() and ((x < 0) | (x > 1)).any(1).sum() == len(case.oob)
    w = gc.world(x, case.bound)  # the fused entries' world coordinates map back exactly
    assert np.array_equal(((w + np.float32(case.bound)) * np.float32(1 / (2 * case.bound))).astype(np.float32), x)
    # 1
    assert (g != 0).all() and np.array_equal(g.astype(np.float16).astype(np.float64), g)
    assert np.array_equal(d["gd"].astype(np.float64), g)
    # 2 (the table's type: the grad's)
    assert np.array_equal(ref.astype(case.dtype).astype(np.float64), ref)
    assert np.isfinite(ref).all()
    # 3
    hashed = gc.hashed_levels(offs, case.D, case.scale, case.H)
    lv = [l for l in range(L) if hashed[l]] or list(range(L))
    nz = sum(int((ref[offs[l]:offs[l + 1]] != 0).any(1).sum()) for l in lv)
    assert nz >= case.min_nonzero, nz
    # 4
    nb = {"suffix": gc.binned_levels(offs), "all": 0, "none": L}[case.term]
    if nb < L:
        assert mag[offs[nb]:].max() < 4.0, float(mag[offs[nb]:].max())
    # 5
    assert gc.window_bound(case, x, g, pid) < 4.0
    # the forced runs are there, live, and of one position
    for r0, m, p in case.runs:
        rows = np.arange(r0, r0 + m)
        rows = rows[pid[rows] >= 0]
        assert (pid[rows] == p).all() and r0 + m <= n


def test_fused_cases_cover_the_routes():
    """The shapes the issue names: a fully binned 2^19 table, 2^22-entry levels
    (1024 bins), an atomic suffix at 2^23, a count ending mid-block, two
    accumulating calls, bound 2, and 40 dense levels of two bins of which
    levels 32..39 merge runs."""
    by = gc.EXACT
    assert gc.binned_levels(by["fused_L16T19"].offsets) == 16
    assert gc.binned_levels(by["fused_L8T22"].offsets) == 8
    o = by["fused_L8T22"].offsets
    assert max(int(o[l + 1] - o[l]) for l in range(8)) == 2 ** 22
    assert gc.binned_levels(by["fused_L6T23"].offsets) == 4
    assert by["fused_L16T19_count_bound2"].count % 512 not in (0,) and by["fused_L16T19_count_bound2"].bound == 2.0
    assert by["fused_L16T19_accumulate"].reps == 2
    c = by["fused_L40S0"]
    o = c.offsets
    assert gc.binned_levels(o) == 40 and not gc.hashed_levels(o, 3, c.scale, c.H).any()
    assert all(-(-int(o[l + 1] - o[l]) // gc.BIN_ENTRIES) == 2 for l in range(40))
    assert all(gc.level_scale(l, c.scale, c.H)[1] <= 256 for l in range(40))  # the run merge is on (kMergeMaxRes)
    # long runs: at row 0, over a wave, a 512-row block and row 16384, and up to the last live row
    runs = by["fused_L16T19"].runs
    assert any(r0 == 0 for r0, m, _ in runs) and any(r0 < 16384 < r0 + m for r0, m, _ in runs)
    assert any(r0 < 512 < r0 + m for r0, m, _ in runs) and any(r0 < 192 < r0 + m for r0, m, _ in runs)
    assert any(r0 + m == 40000 for r0, m, _ in runs) and max(by[k].B for k in by) == 40000
    r0, m, _ = by["fused_L16T19_count_bound2"].runs[-1]
    assert r0 + m == by["fused_L16T19_count_bound2"].count


def test_generic_cases_cover_the_runs():
    """Run lengths 1, 2, 3, 31, 32, 33 and 70; runs from lane 0/1 and up to
    lanes 62/63 (32 points per wave); an outside row inside a run; two cells
    that share one hashed entry; every C and D, all three types."""
    lens = sorted(m for _, m, _ in gc.GENERIC_EXACT[0].runs)
    assert lens == [1, 2, 3, 31, 32, 33, 70]
    for case in gc.GENERIC_EXACT:
        assert any(r0 % 32 == 0 for r0, m, _ in case.runs) and any((r0 + m) % 32 == 0 for r0, m, _ in case.runs)
        assert any(r0 < o < r0 + m for r0, m, _ in case.runs for o in case.oob)
    assert {c.C for c in gc.GENERIC_EXACT} == {1, 2, 4, 8} and {c.D for c in gc.GENERIC_EXACT} == {2, 3, 4, 5}
    assert {np.dtype(c.dtype).name for c in gc.GENERIC_EXACT} == {"float16", "float32", "float64"}
    for case in gc.GENERIC_EXACT:
        if case.nlat != 5:
            continue
        d = gc.exact_data(case.name)
        x, pid, offs = d["x"], d["pid"], d["offs"]
        hashed = gc.hashed_levels(offs, case.D, case.scale, case.H)
        shared = 0
        for l in np.flatnonzero(hashed):
            live = pid >= 0
            ent = gc.corner_entries(x[live], l, offs, case.scale, case.H)
            cell = gc.cells(x[live], l, case.scale, case.H)
            pairs = np.unique(np.stack([ent.ravel(), np.repeat(cell, ent.shape[1])], 1), axis=0)
            shared += int((np.bincount(pairs[:, 0]) > 1).sum())
        assert shared > 0 or not hashed.any(), case.name
    assert any(gc.hashed_levels(c.offsets, c.D, c.scale, c.H).any() for c in gc.GENERIC_EXACT)


def test_corner_entries_match_the_oracle():
    """grid_cases.corner_entries (used above to count shared entries) against
    the oracle's scatter: one row, unit grads, the touched entries."""
    case = gc.EXACT["generic_D3C2_f32"]
    offs = case.offsets
    x = gc.lattice(3, 5)[[7, 62, 93, 124]]
    for i in range(x.shape[0]):
        ref = oracle.grid_encode_backward(np.ones((1, case.L * case.C), np.float32), x[i:i + 1], offs, case.C,
                                          case.scale, case.H)
        for l in range(case.L):
            ent = np.unique(gc.corner_entries(x[i:i + 1], l, offs, case.scale, case.H))
            hit = np.flatnonzero(ref[offs[l]:offs[l + 1], 0])
            assert set(hit) <= set(ent.tolist()) and len(hit) > 0


def test_borrow_dense_level_counts():
    """The forward's chunk lending needs 5 dense levels among 0..7 (L 16, H 16):
    Lego's scale and bound 2 have 5; bound 16's scale 1.6625 has 4, scale 2 has
    3, Lego's scale with a 2^14 table 2 -- the shapes whose grid is sized for
    lending while nothing is lent."""
    def dense(scale, log2T):
        o = oracle.grid_offsets(3, 16, 2, 16, scale, log2T)
        return sum(int(o[l + 1] - o[l]) < int(o[16] - o[15]) for l in range(8))
    assert dense(gc.LEGO_SCALE, 19) == 5 and dense(1.4473, 19) == 5
    assert dense(1.6625, 19) == 4 and dense(2.0, 19) == 3 and dense(gc.LEGO_SCALE, 14) == 2


def test_forward_tables():
    assert len(gc.DIM_CASES) == 16 and {(c[0], c[1]) for c in gc.DIM_CASES} == {(D, C) for D in (2, 3, 4, 5) for C in (1, 2, 4, 8)}
    for k in (2, 3, 4):  # every option value with every D and every C
        for D in (2, 3, 4, 5):
            assert {c[k] for c in gc.DIM_CASES if c[0] == D} == {0, 1}
        for C in (1, 2, 4, 8):
            assert {c[k] for c in gc.DIM_CASES if c[1] == C} == {0, 1}
    e = gc.edge_rows(3)
    assert np.signbit(e).any() and (e == np.nextafter(np.float32(1), np.float32(2))).any() and (e < 0).any()
    x = gc.forward_inputs(300, 3, 1)
    assert x.shape == (300, 3) and not np.isnan(x).any()
