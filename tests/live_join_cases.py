"""Inputs of the tests of the live-row list's join inside the NeRF backward
(ngp_nerf_backward_join_dw, tests/test_gpu_live_join.py): composite inputs whose
live rows are chosen row by row, the per-ray lists the composite leaves for
them, the list their plain concatenation gives, and a numpy restatement of
the kernel's arithmetic (csrc/ffmlp.hip, k_nerf_bwd's join).

A row is live when the composite leaves it a nonzero gradient. Here a dead row
has delta 0 (weight 0 and a zero density gradient: every component +0 or -0)
and a live row delta 0.02 at sigma 1 with colour logits in (-1, 1), a black
target and a black background, so its colour gradient is nonzero; no ray comes
near the early stop (at most 100 live rows: T >= exp(-2)). The GPU test
asserts that the composite's counts are the planned ones.

tests/test_live_join_cases_cpu.py holds the conditions each case is meant to hit.
"""
import functools

import numpy as np

CHUNK = 32                 # rows of a backward chunk
WAVES = 4                  # waves of a backward workgroup
THREADS = 64 * WAVES
RAYS_PER_THREAD = 16       # a thread's ray group in the join
CAP = RAYS_PER_THREAD * THREADS   # 4096 rays: one pass (ngp_nerf_backward_join_max_rays)
MAX_WGS = 256
MAX_CHUNKS = 32            # list chunks a workgroup's LDS list holds
T_THRESH = 1e-4
SCALE = 65536.0
DELTA = 0.02
ROWS_MAX = 64              # dw_rows_max of the small cases: the stash route up to 64 rows


def launch_width(M):
    """Workgroups of the backward over M allocated rows (ffmlp.hip bwd_blocks)."""
    return min(MAX_WGS, -(-(-(-M // CHUNK)) // WAVES))


def light_limit(M, rows_max, stash_rows):
    """The largest count of the stash route (ffmlp.hip dw_rows_limit)."""
    return min(rows_max, stash_rows // CHUNK * CHUNK, launch_width(M) * CHUNK)


class Case:
    """name, counts [N] (live rows per ray), dead [N] (dead rows per ray),
    M (allocated rows), rows_max (dw_rows_max), overflow (the last ray is
    dropped for overflowing M: its planned count is 0)."""

    def __init__(self, name, counts, dead, rows_max=ROWS_MAX, M=None, overflow=False, seed=0):
        self.name, self.rows_max, self.overflow, self.seed = name, rows_max, overflow, seed
        self.counts = np.asarray(counts, np.int64)
        self.dead = np.broadcast_to(np.asarray(dead, np.int64), self.counts.shape).copy()
        self.N = len(self.counts)
        steps = self.counts + self.dead
        used = int(steps.sum())
        self.M = used if M is None else M
        if overflow:
            # the last ray owns rows past the allocation: 3 of its rows lie inside it
            self.M = used - int(steps[-1]) + 3
        assert self.M >= 1

    @property
    def stash_rows(self):
        return max(96, self.rows_max)

    @property
    def G(self):
        return launch_width(self.M)


def _rng(seed):
    return np.random.default_rng(20260000 + seed)


def _small(N, seed, p=(0.45, 0.25, 0.2, 0.1)):
    return _rng(seed).choice(len(p), size=N, p=p)


@functools.lru_cache(maxsize=None)
def cases():
    r = _rng(99)
    out = []
    # N around a thread's ray group and a wave's
    out.append(Case("n1", [5], 2, seed=1))
    for k, N in enumerate((15, 16, 17, 63, 64, 65)):
        out.append(Case(f"n{N}", _small(N, 10 + k), 1, seed=10 + k))
    # the full pass: the bench's shape (about 0.7 live rows per ray of 8), 256 workgroups, stash route
    c4096 = (r.random(CAP) < 0.7).astype(np.int64)
    out.append(Case("n4096_light", c4096, 8 - c4096, rows_max=8192, seed=20))
    # ... and in a small allocation: the slab route with one or two chunks per workgroup
    out.append(Case("n4096_heavy", c4096, 1, rows_max=ROWS_MAX, seed=21))
    # counts
    out.append(Case("all_zero", np.zeros(64), 2, seed=30))
    out.append(Case("last_ray_only", np.r_[np.zeros(64), 1], 1, seed=31))
    out.append(Case("one_each", np.ones(100), 1, rows_max=0, seed=32))
    out.append(Case("one_each_light", np.ones(64), 0, M=300, seed=33))
    out.append(Case("long_ray", np.r_[2, 0, 1, 100, 0, 3, np.zeros(11)], 1, rows_max=0, seed=34))
    out.append(Case("t31", [20, 11], 1, seed=35))
    out.append(Case("t32_on_ray_edge", [16, 16], 1, seed=36))
    out.append(Case("t33_on_ray_edge", [16, 16, 1], 1, seed=37))
    out.append(Case("t33_in_ray", [20, 13], 1, seed=38))
    out.append(Case("overflow_ray", [3, 0, 4, 2, 5], [1, 2, 0, 1, 4], overflow=True, seed=39))
    out.append(Case("gaps", [3, 0, 0, 5, 0, 2, 0, 0, 0, 7, 0, 0, 0, 0, 1, 0, 0, 4, 0, 0], 1, seed=40))
    # regimes: the switch at dw_rows (64 in an allocation of 300 rows: three workgroups) ...
    out.append(Case("at_dw_rows", [30, 30, 4], 1, M=300, seed=50))
    out.append(Case("past_dw_rows", [30, 30, 5], 1, M=300, seed=51))
    # ... and 1, 2, 3, 4 chunks per workgroup on three workgroups (the slab route): whole
    # rounds, the half-chunk rounds (1 or 2 chunks left) and the idle-wave sigma copy (1 or 3)
    for n, total in ((1, 96), (2, 161), (3, 257), (4, 290)):
        cnt = np.full(total // 7, 7)
        cnt = np.r_[cnt, total - cnt.sum()] if total % 7 else cnt
        out.append(Case(f"wg{n}", cnt, 0, rows_max=ROWS_MAX, M=300, seed=60 + n))
    # 5 chunks needs the full launch width: 1026 chunks on 256 workgroups (5 on the first two)
    c5 = np.full(CAP, 8)
    c5[:40] = 9
    out.append(Case("wg5", c5, 0, rows_max=ROWS_MAX, seed=65))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def build(name):
    """The composite's inputs and the planned lists of a case: rays [N, 3] (index,
    first row, rows), live [M] bool, sigma [M], deltas [M, 2], col [M, 16], h
    [M, 16], gt [N, 4], bg [N, 3], cin [M, 32], enc [M, 32], counts [N] (0 for a
    ray dropped for overflow), rows (the list: the concatenation in ray order)."""
    c = case(name)
    r = _rng(1000 + c.seed)
    N, M = c.N, c.M
    steps = c.counts + c.dead
    first = np.concatenate([[0], np.cumsum(steps)[:-1]])
    rays = np.stack([np.arange(N), first, steps], 1).astype(np.int32)
    live = np.zeros(M, bool)
    counts = c.counts.copy()
    per_ray = []
    for i in range(N):
        if c.overflow and i == N - 1:
            counts[i] = 0
            per_ray.append(np.zeros(0, np.int64))
            continue
        pick = np.sort(r.choice(steps[i], c.counts[i], replace=False)) + first[i] if c.counts[i] else np.zeros(0, np.int64)
        live[pick] = True
        per_ray.append(pick)
    f16, f32 = np.float16, np.float32
    col = np.zeros((M, 16), f16)
    col[:, :3] = r.uniform(-1, 1, (M, 3))
    h = np.zeros((M, 16), f16)
    h[:, 0] = r.uniform(-1, 1, M)
    deltas = np.stack([np.where(live, DELTA, 0.0), np.full(M, DELTA)], 1).astype(f32)
    gt = np.zeros((N, 4), f32)
    gt[:, 3] = 1
    d = dict(N=N, M=M, rays=rays, live=live, sigma=np.ones(M, f32), deltas=deltas, col=col, h=h, gt=gt,
             bg=np.zeros((N, 3), f32), cin=r.uniform(0, 1, (M, 32)).astype(f16),
             enc=r.uniform(-1, 1, (M, 32)).astype(f16), counts=counts.astype(np.int32),
             rows=np.concatenate(per_ray).astype(np.int32) if N else np.zeros(0, np.int32), per_ray=per_ray)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def planned_ray_rows(d):
    """ray_rows [M] as the composite leaves it on a zeroed buffer: ray n's live
    rows from its first row on."""
    out = np.zeros(d["M"], np.int32)
    for n, pick in enumerate(d["per_ray"]):
        out[d["rays"][n, 1]:d["rays"][n, 1] + len(pick)] = pick
    return out


# ---- the kernel's arithmetic, restated ----------------------------------------------

def join_prefix(counts, N):
    """First part: thread t sums its 16 rays (rays at or past N count 0), a wave
    scans its 64 thread sums, the four wave totals give the wave bases. Returns
    (pos [CAP]: each ray's position among its wave's rays, wave bases [4], total)."""
    c = np.zeros(CAP, np.int64)
    c[:N] = np.maximum(counts[:N], 0)
    per_thread = c.reshape(THREADS, RAYS_PER_THREAD)
    tsum = per_thread.sum(1).reshape(WAVES, 64)
    incl = np.cumsum(tsum, 1)                        # the wave scan
    first = (incl - tsum).reshape(THREADS)           # the thread's first position in its wave
    pos = (first[:, None] + np.cumsum(per_thread, 1) - per_thread).reshape(CAP)
    wtot = incl[:, -1]
    base = np.concatenate([[0], np.cumsum(wtot)[:-1]])
    return pos, base, int(wtot.sum())


def chunks_of(b, G, total):
    """Workgroup b's chunks b, b + G, ... below the count."""
    nch = -(-total // CHUNK)
    return list(range(b, nch, G))


def runs(b, G, total, light):
    """Whether workgroup b runs the passes: with a chunk in the light regime,
    below the slab rows the reduce reads otherwise (ngp_reduce.h live_slab_rows)."""
    nch = -(-total // CHUNK)
    return b < nch if light else b < min(G, -(-nch // 64) * 64)


def join_entry(p, pos, base, src, ray_rows):
    """Second part, one list position: the wave with the last base <= p, the ray
    with the last pos <= p - base there (a four-way search, 5 rounds), its entry."""
    wv = int(p >= base[1]) + int(p >= base[2]) + int(p >= base[3])
    rel = p - base[wv]
    ray0, lo, q = wv * 64 * RAYS_PER_THREAD, 0, 64 * RAYS_PER_THREAD // 4
    while q:
        lo += q * sum(int(pos[ray0 + lo + k * q] <= rel) for k in (1, 2, 3))
        q //= 4
    return ray_rows[src[ray0 + lo] + (rel - pos[ray0 + lo])]


def join(d, B, G, light_max):
    """The whole launch: (live_rows as the workgroups store it, -1 where no
    workgroup stores; total; owners [chunk] = the workgroups that stored it)."""
    N = d["N"]
    pos, base, total = join_prefix(d["counts"], N)
    src = np.zeros(CAP, np.int64)
    src[:N] = d["rays"][:, 1]
    src[N:] = d["rays"][N - 1, 1]     # (the clamped loads of rays past N)
    ray_rows = planned_ray_rows(d)
    Bc = min(B, total)
    light = light_max > 0 and Bc <= light_max
    out = np.full(d["M"], -1, np.int64)
    owners = {}
    for b in range(G):
        if not runs(b, G, Bc, light):
            continue
        for j, c in enumerate(chunks_of(b, G, Bc)):
            assert j < MAX_CHUNKS
            owners.setdefault(c, []).append(b)
            for p in range(CHUNK * c, min(CHUNK * c + CHUNK, Bc)):
                out[p] = join_entry(p, pos, base, src, ray_rows)
    return out, total, owners
