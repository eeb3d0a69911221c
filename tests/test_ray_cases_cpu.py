"""The ray cases of tests/ray_cases.py do what they claim and every marching
loop over them ends (no GPU): checked with the CPU oracle alone, so
tests/test_gpu_rays.py can demand the identical bits from the device."""
import faulthandler

import numpy as np
import pytest

import ray_cases as rc

NAMES = sorted(rc.CASES)
ORACLE_TIME_LIMIT = 120  # seconds for the serial loop over one case (it takes well under one)


@pytest.fixture(autouse=True)
def _time_limit():
    """A time limit on every test here: the oracle runs the marching loop the
    kernels run, serially in C, where a loop that never ends cannot be
    interrupted from Python. The watchdog thread ends the process instead."""
    faulthandler.dump_traceback_later(ORACLE_TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def test_the_issue_rows_are_present():
    rows = {(b, C, g, mn, H, ms) for b, C, g, mn, H, ms, dens in rc.CASES.values() if dens == 0.3}
    assert rows >= {(1, 1, 0, 0.2, 128, 1024), (1.5, 2, 1 / 128, 0.05, 128, 1024), (2, 2, 1 / 128, 0.05, 128, 1024),
                    (2, 2, 0, 0.0, 64, 1024), (3, 3, 1 / 256, 0.2, 128, 1024), (8, 4, 0, 0.2, 128, 1024),
                    (16, 5, 1 / 64, 0.05, 128, 1024), (16, 5, 1 / 1024, 0.05, 128, 4096)}
    assert [n for n, row in rc.CASES.items() if row[6] == 1.0] == ["b2-full"]
    for name in NAMES:
        c = rc.case(name)
        assert c["N"] == 64 * len(rc.FAMILIES) and tuple(c["slices"]) == rc.FAMILIES
        assert abs((np.unpackbits(c["bits"]).mean()) - c["density"]) < 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_every_loop_ends(name):
    """far is never +inf, finite fars are bounded by the box, and t + dt > t
    along every chain (ray_cases.termination_check); the oracle, the same loop
    run serially, finishes inside this file's time limit."""
    margin = rc.termination_check(name)
    print(f"{name}: smallest step {margin:.0f} ulps of the largest t")
    r = rc.reference(name)
    assert int(r["counter"][0]) == r["total"] and int(r["counter"][1]) == 3 + rc.case(name)["N"]


def test_off_centre_box_and_short_marches_end():
    o = rc.off_centre()
    assert not np.isinf(o["nears"]).any() and not np.isinf(o["fars"]).any()
    assert np.isnan(o["nears"]).any() and np.isnan(o["fars"]).any() and (o["fars"] == rc.FLT_MAX).any()
    lo, hi = np.array(rc.OFF_AABB[:3]), np.array(rc.OFF_AABB[3:])
    assert len(set(hi - lo)) == 3 and np.abs(hi + lo).min() > 0  # non-cubic, off-centre on every axis
    c = rc.case(rc.SHORT_CASE)
    for ms in rc.SHORT_MAX_STEPS:
        r = rc.short_reference(ms)
        dt_min, dt_max = rc.march_consts(dict(c, max_steps=ms))
        assert dt_min > dt_max
        m = int(r["counter"][0])
        assert m > 0 and (r["rays"][:, 2] == ms).sum() >= r["N"] // 2
        # clampf is fminf(hi, fmaxf(lo, x)): with lo > hi the step is hi = dt_max
        assert (r["deltas"][:m, 0] == dt_max).all()


@pytest.mark.parametrize("name", NAMES)
def test_families_hold_what_they_promise(name):
    c, r = rc.case(name), rc.reference(name)
    S, ro, rd, nears, fars = c["slices"], c["rays_o"], c["rays_d"], r["nears"], r["fars"]
    b = np.float32(c["bound"])
    norm = np.linalg.norm(rd.astype(np.float64), axis=1)
    assert np.abs(norm - 1).max() < 1e-6  # unit directions: the marching kernels assume them
    inside = (np.abs(ro) <= b).all(1)
    for f in ("interior", "centre", "diag", "planar", "tiny", "face"):
        assert inside[S[f]].all(), f
    assert inside[S["axis"]].any() and not inside[S["axis"]].all()
    for f in ("away", "miss", "graze"):
        assert not inside[S[f]].any(), f
    # miss: the marker pair; away: near = min_near > far, no marker
    assert (nears[S["miss"]] == rc.FLT_MAX).all() and (fars[S["miss"]] == rc.FLT_MAX).all()
    assert (fars[S["away"]] < nears[S["away"]]).all() and (nears[S["away"]] == np.float32(c["min_near"])).all()
    assert (fars[S["away"]] < 0).all()
    # face: a coordinate exactly on a face; NaN near with finite far, finite near with NaN far, and the marker
    fo, fn, ff = ro[S["face"]], nears[S["face"]], fars[S["face"]]
    assert (np.abs(fo) == b).any(1).all()
    assert (np.isnan(fn) & np.isfinite(ff)).sum() >= 2 and (np.isfinite(fn) & np.isnan(ff)).sum() >= 2
    assert (ff == rc.FLT_MAX).any()
    # axis: one component +-1, the others zeros of both signs
    ad = rd[S["axis"]]
    assert ((np.abs(ad) == 1).sum(1) == 1).all() and ((ad == 0).sum(1) == 2).all()
    zeros = ad[ad == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert (ad == 1).any() and (ad == -1).any()
    # planar: exactly one zero, on each axis in turn
    pd = rd[S["planar"]]
    assert ((pd == 0).sum(1) == 1).all() and (pd == 0).any(0).all()
    # tiny: every listed value, the denormals included, on each axis
    td = rd[S["tiny"]]
    for v in rc.TINY:
        assert (td == np.float32(v)).any(), v
    tiny = np.abs(td) < 1e-7
    assert (tiny.sum(1) == 1).all() and tiny.any(0).all()
    den = (td != 0) & (np.abs(td) < np.finfo(np.float32).tiny)
    with np.errstate(over="ignore"):
        assert den.sum() >= 16 and np.isinf(np.float32(1) / td[den]).all()  # 1 / d overflows: rd = +-inf
    # diag: the longest chords; graze: the three slab entries within 1e-2 bound of each other
    assert (fars[S["diag"]] > 0.9 * 2 * rc.SQRT3 * c["bound"]).all()
    go, gd = ro[S["graze"]].astype(np.float64), rd[S["graze"]].astype(np.float64)
    entry = (np.sign(go) * c["bound"] - go) / gd
    assert (entry.max(1) - entry.min(1) < 1e-2 * c["bound"]).all()
    # centre: origins in the finest cascade's unit cube whatever the bound
    assert (np.abs(ro[S["centre"]]) <= 0.5).all()


@pytest.mark.parametrize("name", NAMES)
def test_cases_are_not_vacuous(name):
    c, r = rc.case(name), rc.reference(name)
    n = r["rays"][:, 2]
    assert (n > 0).mean() >= 0.6, (n > 0).mean()
    for f, s in c["slices"].items():
        if f in ("away", "miss"):
            assert (n[s] == 0).all(), f
        else:
            assert (n[s] > 0).mean() >= 0.25, (f, (n[s] > 0).mean())
    m = r["total"]
    assert np.array_equal(r["rays"][:, 0], np.arange(c["N"]))
    assert np.array_equal(r["rays"][:, 1], np.concatenate([[0], np.cumsum(n)[:-1]]))
    assert np.isfinite(r["xyzs"][:m]).all() and (r["deltas"][:m] > 0).all()
    assert (np.abs(r["xyzs"][:m]) <= c["bound"]).all()
    # the exact zeros and the tiny components reach the output rows unchanged
    assert np.array_equal(np.repeat(c["rays_d"], n, axis=0).view(np.uint32), r["dirs"][:m].view(np.uint32))


def _regimes(c, r):
    dt_min, dt_max = rc.march_consts(c)
    d0 = r["deltas"][:r["total"], 0]
    at_min, at_max = d0 == dt_min, d0 == dt_max
    between = (d0 > dt_min) & (d0 < dt_max)
    assert (at_min | at_max | between).all()
    return at_min, between, at_max


def test_b16_crosses_the_three_dt_regimes():
    c, r = rc.case("b16"), rc.reference("b16")
    at_min, between, at_max = _regimes(c, r)
    assert at_min.sum() > 100 and between.sum() > 100 and at_max.sum() > 100
    owner = np.repeat(np.arange(c["N"]), r["rays"][:, 2])
    held = sum(np.bincount(owner[m], minlength=c["N"]) > 0 for m in (at_min, between, at_max))
    assert (held >= 2).sum() >= 64 and (held == 3).sum() >= 1, ((held >= 2).sum(), (held == 3).sum())


@pytest.mark.parametrize("name", ["b8", "b16-long"])
def test_chains_on_both_sides_of_the_segment_limit(name):
    """b8 (dt_gamma == 0): past 64 segments of 64 indices lane 0 marches alone;
    b16-long: past the 4096 indices the ChainGamma records cover, the same."""
    c, r = rc.case(name), rc.reference(name)
    K = rc.chain_lengths(c, r["nears"], r["fars"])
    n = r["rays"][:, 2]
    # (clear of the limit by 5 %: the kernels bound the length from above before choosing)
    assert ((K > 1.05 * rc.CHAIN_LIMIT) & (n > 0)).sum() >= 64, (K > 1.05 * rc.CHAIN_LIMIT).sum()
    assert ((K > 0) & (K < 0.95 * rc.CHAIN_LIMIT) & (n > 0)).sum() >= 64
    assert (K >= n).all()
    for other in set(NAMES) - {"b8", "b16-long"}:
        o = rc.reference(other)
        assert rc.chain_lengths(rc.case(other), o["nears"], o["fars"]).max() <= rc.CHAIN_LIMIT


@pytest.mark.parametrize("name", ["b8", "b16", "b16-long"])
def test_every_cascade_level_is_sampled(name):
    c, r = rc.case(name), rc.reference(name)
    assert c["C"] >= 4
    levels = np.bincount(rc.sample_levels(c, r["xyzs"][:r["total"]], r["deltas"][:r["total"]]), minlength=c["C"])
    assert levels.shape[0] == c["C"] and (levels >= 100).all(), levels


def test_tie_case_steps_through_a_binade_of_ties():
    """With dt_gamma == 0 the segment starts come from a closed form that takes
    whole runs of equal steps at once, except where t + dt_min is a tie."""
    c, r = rc.case(rc.TIE_CASE), rc.reference(rc.TIE_CASE)
    dt_min, _ = rc.march_consts(c)
    lo, hi = rc.TIE_BINADE
    ratio = float(dt_min) / float(np.spacing(np.float32(lo)))
    assert ratio % 1 == 0.5 and ratio > 1000
    t = np.float32(lo) + np.float32(0.1)
    if not int(t.view(np.uint32)) & 1:
        t = np.nextafter(t, np.float32(hi))
    steps = []
    for _ in range(64):  # from an odd last bit: the first step is one ulp off every later one
        t1 = np.float32(t + dt_min)
        steps.append(float(t1) - float(t))
        t = t1
    assert len(set(steps)) == 2 and len(set(steps[1:])) == 1 and t < hi
    assert abs(steps[0] - steps[1]) == float(np.spacing(np.float32(lo)))
    t0 = rc.ray_t0(c, r["nears"])
    K = rc.chain_lengths(c, r["nears"], r["fars"])
    through = (t0 < lo) & (r["fars"] > lo + 1.0) & (r["rays"][:, 2] > 0)
    assert through.sum() >= 128 and K.max() <= rc.CHAIN_LIMIT  # (the segmented walk, not lane 0 alone)
    # no other dt_gamma == 0 case has such a binade with more than two steps in it
    for name in NAMES:
        if rc.CASES[name][2] == 0 and name != rc.TIE_CASE:
            m = int(rc.march_consts(rc.case(name))[0].view(np.uint32)) & 0x7fffff
            assert m & 1, name


def test_full_bitfield_rays_stop_at_max_steps():
    c, r = rc.case("b2-full"), rc.reference("b2-full")
    assert np.unpackbits(c["bits"]).all()
    n = r["rays"][:, 2]
    assert (n == c["max_steps"]).sum() >= 64 and n.max() == c["max_steps"]
    K = rc.chain_lengths(c, r["nears"], r["fars"])
    assert np.array_equal(n, np.minimum(K, c["max_steps"]))  # every chain index is a sample
    assert (rc.reference("b8")["rays"][:, 2] == rc.case("b8")["max_steps"]).sum() >= 64  # ... and in a sparse case


def test_cut_capacity_drops_whole_rays():
    c, full, cut = rc.case(rc.CUT_CASE), rc.reference(rc.CUT_CASE), rc.reference(rc.CUT_CASE, cut=True)
    M = cut["M"]
    assert 0 < M < full["total"]
    assert np.array_equal(cut["rays"], full["rays"]) and np.array_equal(cut["counter"], full["counter"])
    n, off = cut["rays"][:, 2], cut["rays"][:, 1]
    dropped = (n > 0) & (off + n > M)
    assert dropped.sum() >= 100 and ((n > 0) & ~dropped).sum() >= 100
    straddle = dropped & (off < M)
    assert straddle.sum() == 1  # one ray starts inside the buffer and would run past it: its rows stay zero
    kept = int(off[straddle][0])
    assert np.array_equal(cut["xyzs"][:kept], full["xyzs"][:kept]) and not cut["xyzs"][kept:].any()
    assert not cut["deltas"][kept:].any()


def test_counter_offset_moves_the_rows():
    a, b = rc.reference("b1"), rc.reference("b1", counter0=1000)
    assert np.array_equal(b["rays"][:, 1], a["rays"][:, 1] + 1000) and int(b["counter"][0]) == a["total"] + 1000
    assert not b["xyzs"][:1000].any()
    assert np.array_equal(b["xyzs"][1000:1000 + a["total"]], a["xyzs"][:a["total"]])
