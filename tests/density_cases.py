"""Cases and numpy restatements for the density-grid update's entries
(csrc/density_grid.hip), shared by tests/test_density_cases_cpu.py (which
proves the restatements against torch-CPU and the reference-executed fixture,
and each case table against its own conditions) and
tests/test_gpu_density_entries.py (which holds every entry to them bit for
bit). Imports neither torch nor the GPU.

  points_ref     k_density_points: the reference's fp32 operations in its order
  run_max_ref    tmp_grid[cell] = max(tmp_grid[cell], its points' densities)
  ema_pack_ref   EMA, tmp reset, exact sum, Python-min threshold, packbits
  _draws, _draws_ostat   the counter-RNG draws (draw order / Morton order)

Every case is a pure function of its name, shape and a fixed seed.
"""
import math

import numpy as np

import oracle

F32 = np.float32


# ---- counter RNG and the draws (csrc/density_grid.hip) -----------------------------

def _mix32(x):
    x = np.asarray(x, np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
        x = x ^ (x >> np.uint32(16))
    return x


def _rng_u32(seed, a, b, c):
    """csrc/density_grid.hip rng_u32 (counter RNG), restated in numpy uint32."""
    with np.errstate(over="ignore"):
        inner = _mix32(np.asarray(b, np.uint32) ^ _mix32(np.uint32(c) + np.uint32(0x85ebca6b)))
        return _mix32(np.uint32(seed) ^ _mix32(np.uint32(a) + np.uint32(0x9e3779b9) * inner))


DENSITY_RNG_DOMAIN = 0xd3a5b1c7  # csrc/density_grid.hip kDensityRngDomain


def _draws(seed, update, P, ppc, H, grid=None):
    seed = np.uint32(seed ^ DENSITY_RNG_DOMAIN)
    p = np.arange(P, dtype=np.uint32)
    noise = np.stack([(_rng_u32(seed, update, p, 1 + j) >> np.uint32(8)).astype(np.float32) * np.float32(2 ** -24)
                      for j in range(3)], -1)
    if grid is None:
        return None, noise
    coords = np.stack([_rng_u32(seed, update, p, 8 + j) % np.uint32(H) for j in range(3)], -1).astype(np.int32)
    cas, k = p // ppc, p % ppc
    for c in range(grid.shape[0]):
        occ = np.nonzero(grid[c] > 0)[0].astype(np.int32)
        sel = (cas == c) & (k >= ppc // 2)
        if occ.size:
            cells = occ[_rng_u32(seed, update, p[sel], 7) % np.uint32(occ.size)]
            coords[sel] = oracle.morton3D_invert(cells)
    return coords, noise


def _exp_fixed(r):
    """csrc/density_grid.hip exp_fixed: -ln(u) of u = ((r >> 8) + 1) / 2^24 in
    2^-32 fixed point, the same IEEE double operations in the same order."""
    v = (np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.uint64) + np.uint64(1)
    e = np.array([int(x).bit_length() - 1 for x in v.ravel()], np.int64).reshape(v.shape)
    m = v.astype(np.float64) / np.exp2(e.astype(np.float64))
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    q = np.full_like(s, 1.0 / 15.0)
    for c in (1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0, 1.0):
        q = q * s2 + c
    lnm = 2.0 * s * q
    E = (24 - e).astype(np.float64) * 0.6931471805599453 - lnm
    return np.where(E > 0, (np.maximum(E, 0) * 4294967296.0).astype(np.uint64), np.uint64(0))


def _draws_ostat(seed, update, C, H, grid):
    """ngp_density_grid_draw_sorted's draws (cells per point, uniform half then
    occupied half per cascade) restated in numpy: uniform order statistics
    S_k / S_N from the prefix sums of N + 1 fixed-point exponentials."""
    seed = np.uint32(seed ^ DENSITY_RNG_DOMAIN)
    H3, N = H ** 3, H ** 3 // 4
    j = np.arange(N + 1, dtype=np.uint32)
    cells = []
    for cas in range(C):
        occ = np.nonzero(grid[cas] > 0)[0].astype(np.int64)
        for half in range(2):
            E = _exp_fixed(_rng_u32(seed, update, j, 16 + 2 * cas + half))
            S = np.cumsum(E, dtype=np.uint64)
            t = S[:N].astype(np.float64) / np.float64(S[N])
            if half and occ.size:
                cells.append(occ[np.minimum(np.floor(t * occ.size), occ.size - 1).astype(np.int64)])
            else:
                cells.append(np.minimum(np.floor(t * H3), H3 - 1).astype(np.int64))
    cells = np.concatenate(cells)
    _, noise = _draws(int(seed ^ np.uint32(DENSITY_RNG_DOMAIN)), update, C * 2 * N, 2 * N, H)
    return oracle.morton3D_invert(cells.astype(np.int32)).astype(np.int32), noise, cells


# ---- restatements --------------------------------------------------------------------

def cascade_scales(C, H, bound):
    """csrc/density_grid.hip cascade_scales: bound_c = min(2^c, bound) and
    hgs = bound_c / H in Python floats, (bound_c - hgs) and hgs rounded to fp32.
    `bound` is the fp32 value the entry receives."""
    b = float(F32(bound))
    s, h = [], []
    for c in range(C):
        bc = min(float(2 ** c), b)
        hgs = bc / H
        s.append(F32(bc - hgs))
        h.append(F32(hgs))
    return np.array(s, F32), np.array(h, F32)


def points_ref(coords, noise, ppc, C, H, bound):
    """k_density_points in numpy. coords int32 [C * ppc, 3] or None (every cell
    of each cascade, point i of a cascade = the cell of Morton code i, whose
    noise row is the cell's meshgrid(x, y, z, 'ij') row); noise fp32 [P, 3].
    Returns xyz fp32 [P, 3], index int32 [P] = cascade * H^3 + morton3D."""
    H3 = H ** 3
    P = C * ppc
    noise = np.asarray(noise, F32)
    cas = np.arange(P) // ppc
    if coords is None:
        assert ppc == H3
        c = oracle.morton3D_invert((np.arange(P) % ppc).astype(np.int32)).astype(np.int64)
        row = cas * ppc + (c[:, 0] * H + c[:, 1]) * H + c[:, 2]
        noise = noise[row]
    else:
        c = np.asarray(coords).astype(np.int64)
        noise = noise[:P]
    s, h = cascade_scales(C, H, bound)
    inv = F32(1.0) / F32(H - 1)
    x = F32(2.0) * c.astype(F32)
    x = x * inv
    x = x - F32(1.0)
    x = x * s[cas][:, None]
    j = noise * F32(2.0)
    j = j - F32(1.0)
    j = j * h[cas][:, None]
    xyz = x + j
    assert xyz.dtype == F32
    idx = (cas * H3 + oracle.morton3D(c.astype(np.int32)).astype(np.int64)).astype(np.int32)
    return xyz, idx


def run_max_ref(tmp, sigma, idx):
    """The per-cell maximum of the points' densities folded into `tmp` (a copy)."""
    out = np.array(tmp, F32).reshape(-1).copy()
    np.maximum.at(out, np.asarray(idx, np.int64), np.asarray(sigma, F32))
    return out


def ema_pack_ref(grid, tmp, decay, density_thresh):
    """ngp_density_grid_ema_pack: the reference's EMA (renderer.py:581-583),
    mean (:584) and packbits threshold (:588-589) with numpy / Python floats.
    Returns dict(grid, tmp, sum, mean, thresh, bits)."""
    g = np.array(grid, F32).reshape(-1)
    t = np.array(tmp, F32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        valid = (g >= 0) & (t >= 0)
        # np.maximum(g * decay, t), NaN propagating, written as a select: where the
        # two are equal zeros of opposite sign np.maximum's pick depends on its
        # SIMD path (torch's on the operand order); the kernel keeps tmp's
        gd = g * F32(decay)
        mx = np.where(np.isnan(gd) | np.isnan(t), F32(np.nan), np.where(gd > t, gd, t))
        new = np.where(valid, mx, g).astype(F32)
        clamped = np.maximum(new, F32(0))  # clamp(min=0): NaN propagates
        total = math.fsum(float(v) for v in clamped)
        mean = F32(total / g.size)
        thresh = F32(min(float(mean), density_thresh))
        bits = np.packbits(new > thresh, bitorder="little")
    return dict(grid=new, tmp=np.full_like(t, -1.0), sum=total, mean=mean, thresh=thresh, bits=bits)


def sum_bound(n):
    """Relative error of a sum of n non-negative fp64 terms added in any
    order: each of the n - 1 adds rounds by at most 2^-53 relative to a
    partial sum that is at most the total."""
    return n * 2.0 ** -53


def mean_is_robust(total, n):
    """The fp32 mean is the same for every sum within sum_bound of `total`
    (so the threshold, and every bit, cannot depend on the summation order)."""
    if not math.isfinite(total):
        return True
    e = sum_bound(n)
    return F32(total * (1 - e) / n) == F32(total * (1 + e) / n)


# ---- grids for the draws ---------------------------------------------------------------

DRAW_KINDS = ("empty_cascade", "first_cell", "last_cell", "full")
DRAW_H = (4, 8, 16)
DRAW_C = (1, 2, 3)


def empty_cascade_of(C, H):
    """Which cascade of the 'empty_cascade' grid holds nothing above 0."""
    return (H // 4) % C


def draw_grid(kind, C, H):
    """fp32 [C, H^3]. empty_cascade: one cascade of 0.0 / -0.0 / -1 / NaN /
    negative cells beside ~30 % occupied ones; first_cell / last_cell: one
    occupied cell (index 0 / H^3 - 1) per cascade; full: every cell occupied."""
    H3 = H ** 3
    rng = np.random.default_rng(1000 * DRAW_KINDS.index(kind) + 10 * H + C)
    if kind == "empty_cascade":
        g = (rng.random((C, H3)) - 0.7).astype(F32)
        dead = np.array([0.0, -0.0, -1.0, np.nan, -0.5], F32)
        row = dead[rng.integers(0, dead.size, H3)]
        row[:4] = dead[:4]
        g[empty_cascade_of(C, H)] = row
        return g
    if kind in ("first_cell", "last_cell"):
        g = np.array([0.0, -1.0, -0.0], F32)[rng.integers(0, 3, (C, H3))]
        g[:, 0 if kind == "first_cell" else H3 - 1] = F32(0.5)
        return g
    assert kind == "full"
    return (rng.random((C, H3)) + 0.1).astype(F32)


CARRY_C, CARRY_H = 2, 128


def carry_grid():
    """H = 128, C = 2: the only occupied cells lie in the 1024-cell blocks
    numbered >= 1024 of cascade 1 (the occupied-cell scan strides 1024 block
    counts at a time and carries the running total into the second stride)."""
    H3 = CARRY_H ** 3
    rng = np.random.default_rng(77)
    g = np.zeros((CARRY_C, H3), F32)
    first = 1024 * 1024
    g[1, first:] = np.where(rng.random(H3 - first) < 0.03, F32(0.75), F32(0.0))
    g[1, first] = g[1, H3 - 1] = F32(0.75)
    return g


# ---- run-max cases ---------------------------------------------------------------------

RUN_PATTERNS = ("ostat", "single", "distinct", "both_halves", "boundary")
RUN_H = (4, 8)
RUN_C = (1, 2, 3)
SIGMA_PALETTE = np.array([0.0, 1e-40, 0.5, 0.5, 2.0, 2.0, 1e30, np.inf], F32)  # +0, a denormal, ties, huge, inf
TMP_PALETTE = np.array([-1.0, 0.25, 3e38], F32)  # unset, below most densities, above every finite one
SPLIT_CASE = ("boundary", 2, 4)      # every [0, s) + [s, P)
THREE_WAY_CASE = ("both_halves", 3, 8)
LONG_SLICE = ("ostat", 3, 8, 100, 700)  # 600 points: more than 256, not a multiple


def _sorted_cells(rng, n, lo, hi):
    return np.sort(rng.integers(lo, hi, n))


def run_max_case(pattern, C, H):
    """idx int32 [C * 2N] (cascade * H^3 + cell, sorted inside each half of N =
    H^3 / 4 points), sigma fp32 [C * 2N], tmp fp32 [C * H^3]."""
    H3, N = H ** 3, H ** 3 // 4
    rng = np.random.default_rng(500 * RUN_PATTERNS.index(pattern) + 10 * H + C)
    X = H3 // 2
    halves = []
    if pattern == "ostat":
        grid = (rng.random((C, H3)) - 0.7).astype(F32)
        cells = _draws_ostat(11, 3, C, H, grid)[2]
    else:
        for cas in range(C):
            if pattern == "single":  # the occupied half of each cascade is one cell: a run of N
                halves += [_sorted_cells(rng, N, 0, H3), np.full(N, (5 + 9 * cas) % H3)]
            elif pattern == "distinct":
                halves += [np.arange(N) * 4, np.arange(N) * 4 + 1 + cas % 3]
            elif pattern == "both_halves":  # cell X: a run of 3 in the uniform half, of 4 in the occupied half
                halves += [np.sort(np.concatenate([[X] * 3, rng.integers(0, H3, N - 3)])),
                           np.sort(np.concatenate([[X] * 4, rng.integers(0, H3, N - 4)]))]
            else:  # boundary: X's run ends the first half exactly, and another run of X opens the second
                halves += [np.concatenate([_sorted_cells(rng, N - 3, 0, X), [X] * 3]),
                           np.concatenate([[X] * 2, _sorted_cells(rng, N - 2, X + 1, H3)])]
        cells = np.concatenate(halves)
    idx = (np.repeat(np.arange(C), 2 * N) * H3 + cells).astype(np.int32)
    sigma = SIGMA_PALETTE[rng.integers(0, SIGMA_PALETTE.size, idx.size)]
    tmp = TMP_PALETTE[rng.integers(0, TMP_PALETTE.size, C * H3)]
    return idx, sigma, tmp


def run_length_at(idx, N, s):
    """Length of the run of equal indices (inside one half) that the slice
    boundary s cuts strictly inside, or 0 when s cuts no run."""
    if s <= 0 or s >= idx.size or s % N == 0 or idx[s - 1] != idx[s]:
        return 0
    a = b = s
    while a - 1 >= (s // N) * N and idx[a - 1] == idx[s]:
        a -= 1
    while b < (s // N + 1) * N and idx[b] == idx[s]:
        b += 1
    return b - a


def three_way_cuts(idx, N):
    """Two uneven cuts: the first strictly inside the first run of >= 3."""
    s1 = next(s for s in range(1, idx.size) if run_length_at(idx, N, s) >= 3)
    s2 = idx.size - 101
    assert 0 < s1 < s2 < idx.size
    return s1, s2


# ---- EMA + packbits cases ---------------------------------------------------------------

EMA_H = (2, 4, 8)
EMA_C = (1, 2, 3)
EMA_NAMES = ("cross_finite", "cross_inf", "cross_nan", "tie_mean", "tie_thresh")
DECAY = 0.95
DENORMAL = F32(1e-40)
ROUNDS = F32(3.0)  # 3 * fp32(0.95) is not an fp32 value: the product rounds
GRID_VALUES = np.array([-1.0, 0.0, DENORMAL, ROUNDS, 1e30, np.inf, np.nan], F32)
TMP_KINDS = ("unset", "negzero", "zero", "below", "equal", "above", "inf", "nan")


def tmp_value(g, kind):
    """The scratch value of `kind` for a cell holding g: below / equal / above
    are relative to fp32(g * fp32(decay)) (1.0 where g has no positive product)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        base = F32(g) * F32(DECAY) if g > 0 else F32(1.0)
        return F32({"unset": -1.0, "negzero": -0.0, "zero": 0.0, "inf": np.inf, "nan": np.nan,
                    "below": base * F32(0.5) if np.isfinite(base) else F32(1.0),
                    "equal": base,
                    "above": base * F32(2.0) if np.isfinite(base) else np.inf}[kind])


def ema_case(name, C, H):
    """dict(grid [C * H^3], tmp [C * H^3], decay, thresh)."""
    n = C * H ** 3
    if name.startswith("cross"):
        ng, nt = {"cross_finite": (5, 6), "cross_inf": (6, 7), "cross_nan": (7, 8)}[name]
        combos = [(g, k) for g in GRID_VALUES[:ng] for k in TMP_KINDS[:nt]]
        if name != "cross_finite":  # NaN cells, then the other non-finite members, first: present at every size
            combos.sort(key=lambda gk: 0 if np.isnan(gk[0]) else 1 if np.isinf(gk[0]) or gk[1] in ("inf", "nan") else 2)
        else:
            combos = combos[(7 * C + H) % len(combos):] + combos[:(7 * C + H) % len(combos)]
        pick = [combos[i % len(combos)] for i in range(n)]
        grid = np.array([g for g, _ in pick], F32)
        tmp = np.array([tmp_value(g, k) for g, k in pick], F32)
        return dict(grid=grid, tmp=tmp, decay=DECAY, thresh=2.5)
    if name == "tie_mean":
        # the updated grid is -1 0 2 2 4 4 2 2 over and over: sum 16 per 8 cells in
        # small integers (exact in any order), mean exactly 2.0 = the threshold
        grid = np.tile(np.array([-1, 0, 1, 1, 1, 1, 1, 1], F32), n // 8)
        tmp = np.tile(np.array([5, 0, 2, 2, 4, 4, 2, 2], F32), n // 8)
        return dict(grid=grid, tmp=tmp, decay=DECAY, thresh=10.0)
    assert name == "tie_thresh"
    # density_thresh 0.01 (not an fp32 value) below the mean: the threshold is
    # fp32(0.01); cells equal to it, one ulp either side of it, and large ones
    f = F32(0.01)
    vals = np.array([f, np.nextafter(f, F32(1)), np.nextafter(f, F32(0)), 5.0, f, 0.0, -1.0, 5.0], F32)
    via_tmp = np.tile(np.array([1, 1, 1, 1, 0, 1, 0, 0], bool), n // 8)
    vals = np.tile(vals, n // 8)
    grid = np.where(via_tmp, F32(0), vals).astype(F32)   # max(0 * decay, tmp) = tmp
    tmp = np.where(via_tmp, vals, F32(-1)).astype(F32)   # or the cell unchanged (no decay)
    return dict(grid=grid, tmp=tmp, decay=DECAY, thresh=0.01)


BIG_C, BIG_H = 1, 128


def ema_big_case():
    """H = 128, C = 1: n = 2^21 = two passes of k_density_ema's outer loop
    (1024 blocks x 256 threads x 4 cells a pass). Threshold = the mean."""
    n = BIG_C * BIG_H ** 3
    rng = np.random.default_rng(2024)
    grid = (rng.random(n) * 2).astype(F32)
    grid[rng.random(n) < 0.1] = -1
    tmp = (rng.random(n) * 2).astype(F32)
    tmp[rng.random(n) < 0.5] = -1
    return dict(grid=grid, tmp=tmp, decay=DECAY, thresh=10.0)
