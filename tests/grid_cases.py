"""Case tables and input generators for the grid encoder's route tests
(tests/test_grid_cases_cpu.py, tests/test_gpu_grid_routes.py). numpy and the
CPU oracle only: importable without a GPU.

Exact-sum inputs (DESIGN.md §5 "Grid encoder: the inputs and the margin").
With a per-level scale of 2 or 1 and an even base resolution H the kernels'
`scale` (2^l * H - 1 or H - 1) is an odd integer. Rows sit on the lattice
{0, 1/4, 1/2, 3/4, 1}^D ({0, 1/2, 1}^D for D 4 and 5), so `x * scale + 0.5` is
exact, every interpolation weight is a multiple of 2^-6 (4^-D, or 2^-D on the
coarse lattice) and with output grads +-{1, 2, 3} * 2^-3 every term w * g is a
multiple of 2^-9. The visits of one lattice position alternate in sign, each
+- pair with one magnitude, so every contiguous window of rows at one
position sums to at most two terms and every table entry's total stays small:
all partial sums, in any order and any grouping, are fp16 numbers, and a
backward kernel must reproduce the float64 scatter BIT FOR BIT. Volume comes
from cancellation (the binned backward drops rows whose grads are zero, so
zero padding would test nothing): every grad of every row is nonzero.
"""
import functools

import numpy as np

import oracle

LEGO_SCALE = float(np.exp2(np.log2(2048 / 16) / 15))

# the binned backward's plan (gridencoder.hip make_bin_plan): bins of 2^12
# entries; levels past 1024 bins, or past 11776 bins in all, go term by term
BIN_ENTRIES, MAX_BINS_LEVEL, MAX_BINS_TOTAL = 4096, 1024, 11776
PRIMES = np.array([1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737], dtype=np.uint64)


def binned_levels(offs):
    """Levels [0, n) the fused backward bins; the rest add term by term in fp16."""
    bins = 0
    for l in range(len(offs) - 1):
        nb = -(-int(offs[l + 1] - offs[l]) // BIN_ENTRIES)
        if nb > MAX_BINS_LEVEL or bins + nb > MAX_BINS_TOTAL:
            return l
        bins += nb
    return len(offs) - 1


def level_scale(l, scale, H):
    """The kernels' per-level `scale` and resolution (gridencoder.hip make_levels)."""
    s = np.float32(np.float32(np.exp2(np.float64(np.float32(l) * np.float32(np.log2(scale))))) * np.float32(H)) - np.float32(1)
    return float(s), int(np.ceil(s)) + 1


def hashed_levels(offs, D, scale, H, align_corners=False):
    out = []
    for l in range(len(offs) - 1):
        _, res = level_scale(l, scale, H)
        out.append(float(res if align_corners else res + 1) ** D > int(offs[l + 1] - offs[l]))
    return np.array(out)


def lattice(D, n):
    g = np.arange(n, dtype=np.float32) / np.float32(n - 1)
    return np.stack(np.meshgrid(*([g] * D), indexing="ij"), -1).reshape(-1, D)


def cells(x, l, scale, H):
    """Integer cell (floor(x * scale + 0.5) per axis) of each row on level l, as one key per row."""
    s, _ = level_scale(l, scale, H)
    pg = np.floor(x.astype(np.float64) * s + 0.5).astype(np.int64)
    key = np.zeros(x.shape[0], np.int64)
    for d in range(x.shape[1]):
        key = key * (1 << 21) + pg[:, d]
    return key


def corner_entries(x, l, offs, scale, H):
    """[n, 2^D] table entry (within the level) of every corner of every row,
    gridtype hash, align_corners off (gridencoder.hip grid_index / fast_hash)."""
    s, res = level_scale(l, scale, H)
    hs = int(offs[l + 1] - offs[l])
    D = x.shape[1]
    pg = np.floor(x.astype(np.float64) * s + 0.5).astype(np.uint64)
    out = np.empty((x.shape[0], 1 << D), np.int64)
    for idx in range(1 << D):
        pl = pg + np.array([(idx >> d) & 1 for d in range(D)], dtype=np.uint64)
        stride, index, d = 1, np.zeros(x.shape[0], np.uint64), 0
        while d < D and stride <= hs:
            index = (index + pl[:, d] * np.uint64(stride)) & np.uint64(0xffffffff)
            stride *= res + 1
            d += 1
        if stride > hs:
            index = np.zeros(x.shape[0], np.uint64)
            for d in range(D):
                index ^= (pl[:, d] * PRIMES[d]) & np.uint64(0xffffffff)
        out[:, idx] = (index % np.uint64(hs)).astype(np.int64)
    return out


class ExactCase:
    """One exact-sum input set. runs: (first row, length, lattice position)
    forced same-position runs; oob: rows put outside the unit box; count: live
    rows (None: all); reps: accumulating calls; term: "suffix" (the fused
    backward: the levels past the binned prefix add term by term in fp16),
    "all" (the generic fp16 kernel) or "none" (fp32 / fp64 sums)."""

    def __init__(self, name, D, C, L, H, scale, log2T, B, runs, seed, nlat=5, mags=(1, 2, 3), oob=(), count=None,
                 bound=1.0, reps=1, term="suffix", dtype=np.float16, min_nonzero=1000):
        self.name, self.D, self.C, self.L, self.H, self.scale, self.log2T, self.B = name, D, C, L, H, scale, log2T, B
        self.runs, self.seed, self.nlat, self.mags, self.oob, self.count = runs, seed, nlat, mags, tuple(oob), count
        self.bound, self.reps, self.term, self.dtype, self.min_nonzero = bound, reps, term, dtype, min_nonzero

    def __repr__(self):
        return self.name

    @property
    def n(self):
        return self.B if self.count is None else self.count

    @property
    def offsets(self):
        return oracle.grid_offsets(self.D, self.L, self.C, self.H, self.scale, self.log2T)


def exact_inputs(case):
    """x [B, D] float32 on the lattice (rows in case.oob outside the box),
    g [B, L*C] float64 output grads (exact in fp16), pid [B] lattice position
    of each row (-1: outside)."""
    rng = np.random.default_rng(case.seed)
    pts = lattice(case.D, case.nlat)
    P, B = pts.shape[0], case.B
    pid = np.full(B, -2, np.int64)
    for r0, n, p in case.runs:
        assert (pid[r0:r0 + n] == -2).all() and r0 + n <= B, (case.name, r0)
        pid[r0:r0 + n] = p % P
    pid[list(case.oob)] = -1
    free = np.flatnonzero(pid == -2)
    R = free.size
    # every position an odd number of free visits where the rows allow it, so
    # that its +- pairs leave one term standing (a nonzero expected value)
    if R <= P:
        fill = rng.permutation(P)[:R]
    else:
        cnt = np.ones(P, np.int64) + 2 * rng.multinomial((R - P) // 2, np.full(P, 1.0 / P))
        cnt[rng.integers(P)] += (R - P) % 2
        fill = rng.permutation(np.repeat(np.arange(P), cnt))
    pid[free] = fill
    x = np.where(pid[:, None] >= 0, pts[np.maximum(pid, 0)], np.float32(0.5)).astype(np.float32)
    x[pid < 0, 0] = np.float32(1.5)
    # visit index of each in-box row among the rows of its position, in row order
    valid = np.flatnonzero(pid >= 0)
    order = valid[np.argsort(pid[valid], kind="stable")]
    sp = pid[order]
    first = np.flatnonzero(np.r_[True, sp[1:] != sp[:-1]])
    visit = np.empty(B, np.int64)
    visit[order] = np.arange(order.size) - np.repeat(first, np.diff(np.r_[first, order.size]))
    K = case.L * case.C
    g = np.full((B, K), 0.125)
    _, inv = np.unique(pid[valid] * B + (visit[valid] >> 1), return_inverse=True)
    mags = rng.choice(np.array(case.mags, np.float64), (int(inv.max()) + 1, K)) * 0.125
    g[valid] = (1.0 - 2.0 * (visit[valid] & 1))[:, None] * mags[inv]
    return x, g, pid


def world(x, bound):
    """World coordinates of normalised lattice rows (exact for bound 1 and 2)."""
    return (x * np.float32(2 * bound) - np.float32(bound)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact_data(name):
    """Inputs and float64 references of one case, computed once and shared
    read-only: x, g (float64) and gd (g in the case's dtype), pid, offs, ref
    (scatter of the live rows, times reps), mag (scatter of |g|, times reps)."""
    case = EXACT[name]
    x, g, pid = exact_inputs(case)
    n, offs = case.n, case.offsets
    gd = g.astype(case.dtype)
    kw = dict(offsets=offs, C=case.C, per_level_scale=case.scale, H=case.H)
    ref = case.reps * oracle.grid_encode_backward(gd[:n], x[:n], **kw)
    mag = case.reps * oracle.grid_encode_backward(np.abs(g[:n]), x[:n], **kw)
    for a in (x, g, gd, pid, ref, mag):
        a.setflags(write=False)
    return dict(x=x, g=g, gd=gd, pid=pid, ref=ref, mag=mag, offs=offs)


def window_bound(case, x, g, pid):
    """Upper bound on |sum of g| over any contiguous window of live rows that
    share a cell on some level (what an in-wave run merge may add up before
    its single rounding): per column, the spread of the prefix sums taken from
    the start of each maximal same-cell run."""
    n = case.n
    live = np.flatnonzero(pid[:n] >= 0)
    worst = 0.0
    for l in range(case.L):
        key = cells(x[live], l, case.scale, case.H)
        start = np.r_[True, (key[1:] != key[:-1]) | (np.diff(live) != 1)]
        gl = g[live][:, l * case.C:(l + 1) * case.C]
        cs = np.cumsum(gl, 0)
        base = np.vstack([np.zeros((1, case.C)), cs[:-1]])[np.flatnonzero(start)]
        rel = cs - np.repeat(base, np.diff(np.r_[np.flatnonzero(start), live.size]), 0)
        worst = max(worst, float(max(rel.max(), 0.0) - min(rel.min(), 0.0)))
    return worst


def _runs(B, n, pos=(0, 124, 62, 31, 93), length=70):
    """Long runs at row 0 (over the wave boundary at 64), over a later wave
    boundary (192), a 512-row block boundary, row 16384 and up to the last
    live row, where the batch has those rows."""
    starts = [0, 192 - length // 2, 512 - length // 2 - 3, 16384 - length // 2 - 1, n - length]
    out = []
    for s, p in zip(starts, pos):
        if s >= 0 and s + length <= n and all(s >= a + m or s + length <= a for a, m, _ in out):
            out.append((s, length, p))
    return out


# lattice position ids, 5^3 lattice: 0 and 124 are corners of the box (every
# weight 1/8 there), 62 is the centre (one corner takes weight 1)
FUSED_EXACT = [
    ExactCase("fused_L16T19", 3, 2, 16, 16, 2.0, 19, 40000, _runs(40000, 40000), 1, oob=(17, 16400)),
    ExactCase("fused_L16T19_count_bound2", 3, 2, 16, 16, 2.0, 19, 40000, _runs(40000, 31007), 2, oob=(5, 600),
              count=31007, bound=2.0),
    ExactCase("fused_L16T19_accumulate", 3, 2, 16, 16, 2.0, 19, 40000, _runs(40000, 33333), 3, oob=(100,), count=33333,
              reps=2),
    ExactCase("fused_L8T22", 3, 2, 8, 16, 2.0, 22, 30000, _runs(30000, 30000), 4, oob=(1, 16383)),
    # 2^23-entry levels (4, 5) are past the binned prefix: term-by-term fp16 atomics, so few rows
    ExactCase("fused_L6T23", 3, 2, 6, 16, 2.0, 23, 1100, _runs(1100, 1100, pos=(0, 124, 4, 0, 120), length=66), 5,
              oob=(700,)),
    ExactCase("fused_L4H8T12", 3, 2, 4, 8, 2.0, 12, 513, _runs(513, 513), 6, oob=(200,)),
    # scale 1: 40 dense levels of two bins each, levels 32..39 binned with the run merge on
    ExactCase("fused_L40S0", 3, 2, 40, 16, 1.0, 19, 17000, _runs(17000, 17000), 7, oob=(3, 16390)),
]

# the generic kernel (k_grid_bwd): 32 points per wave, two lanes per point.
# Runs of 1, 2, 3, 31, 32, 33 and 70 rows: from lane 0/1 (row 32: a whole
# wave; row 64: 31 rows), up to lanes 62/63 (rows 253..255), over the
# 128-point block's end (row 96: 33 rows) and over two wave boundaries (row
# 150: 70 rows, with an outside row inside it; at position 0, a corner of the
# box, where every weight is 2^-D, to keep the fp16 cases' sum of |terms| low)
_GRUNS = [(32, 32, 3), (64, 31, 1), (96, 33, 2), (150, 70, 0), (253, 3, 4), (256, 2, 5), (300, 1, 6)]
_GRUNS3 = [(32, 32, 8), (64, 31, 2), (96, 33, 6), (150, 70, 0), (253, 3, 4), (256, 2, 5), (300, 1, 1)]


def _generic(name, D, C, L, H, scale, log2T, dtype, seed, nlat=5, mags=(1, 2, 3), min_nonzero=100, B=640):
    runs = _GRUNS if nlat == 5 else _GRUNS3
    return ExactCase(name, D, C, L, H, scale, log2T, B, runs, seed, nlat=nlat, mags=mags, oob=(180, min(400, B - 9)),
                     term="all" if dtype == np.float16 else "none", dtype=dtype, min_nonzero=min_nonzero)


GENERIC_EXACT = [
    _generic("generic_D3C2_f16", 3, 2, 5, 4, 2.0, 10, np.float16, 11, mags=(1,), min_nonzero=400),
    _generic("generic_D3C2_f32", 3, 2, 5, 4, 2.0, 10, np.float32, 12, min_nonzero=400),
    _generic("generic_D3C4_f64", 3, 4, 4, 4, 2.0, 9, np.float64, 13, min_nonzero=300),
    _generic("generic_D2C1_f16", 2, 1, 5, 8, 2.0, 10, np.float16, 14, mags=(1,), min_nonzero=60, B=320),
    _generic("generic_D2C8_f32", 2, 8, 6, 2, 2.0, 8, np.float32, 15, min_nonzero=60),
    _generic("generic_D3C8_f16", 3, 8, 3, 4, 2.0, 10, np.float16, 16, mags=(1,), min_nonzero=100),
    _generic("generic_D3C1_f64", 3, 1, 5, 4, 1.0, 6, np.float64, 17, min_nonzero=30),
    _generic("generic_D4C1_f32", 4, 1, 4, 2, 2.0, 10, np.float32, 18, nlat=3, min_nonzero=200),
    _generic("generic_D4C4_f16", 4, 4, 3, 4, 2.0, 10, np.float16, 19, nlat=3, mags=(1,), min_nonzero=200),
    _generic("generic_D5C2_f16", 5, 2, 3, 4, 2.0, 12, np.float16, 20, nlat=3, mags=(1,), min_nonzero=200),
    _generic("generic_D5C1_f64", 5, 1, 3, 2, 2.0, 11, np.float64, 21, nlat=3, min_nonzero=200),
]

EXACT = {c.name: c for c in FUSED_EXACT + GENERIC_EXACT}


# ---- forward routes -----------------------------------------------------------

def edge_rows(D):
    """Rows a forward must encode bit for bit: 0, -0.0, 1, the float after 1
    and the float before 0 (both outside the box), each on one axis with the
    others inside. (NaN is excluded: `(uint32_t)floorf(NaN)` is implementation-
    defined in the kernel and in the C oracle alike.)"""
    one, zero = np.float32(1), np.float32(0)
    vals = [zero, -zero, one, np.nextafter(one, np.float32(2)), np.nextafter(zero, np.float32(-1))]
    rows = []
    for i, v in enumerate(vals):
        r = np.full(D, np.float32(0.375))
        r[i % D] = v
        rows.append(r)
        rows.append(np.full(D, v))
    return np.array(rows, np.float32)


def forward_inputs(B, D, seed, nlat=5):
    """Random rows, the edge rows, and lattice rows (x * scale + 0.5 an exact
    integer or half-integer for an odd integer scale)."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, D), dtype=np.float32)
    e = edge_rows(D)
    x[:e.shape[0]] = e
    lat = lattice(D, nlat)
    m = min(lat.shape[0], B - e.shape[0] - 8)
    x[e.shape[0]:e.shape[0] + m] = lat[rng.permutation(lat.shape[0])[:m]]
    return x


LEVEL_COUNTS = [1, 2, 7, 8, 9, 15, 17, 24, 25, 33, 64]

# D, C, gridtype, align_corners, interp: every (D, C) once, the options spread
# over the table (each value of each option with every D and with every C)
DIM_CASES = [(D, C, (i + j) % 2, (i + j // 2) % 2, (i // 2 + j) % 2)
             for i, D in enumerate((2, 3, 4, 5)) for j, C in enumerate((1, 2, 4, 8))]


def forward_table(D, L, C, H, scale, log2T, seed, align_corners=False):
    offs = oracle.grid_offsets(D, L, C, H, scale, log2T, align_corners)
    emb = (np.random.default_rng(seed).standard_normal((int(offs[-1]), C)) * 0.1).astype(np.float32)
    return offs, emb
