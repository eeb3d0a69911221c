"""Inputs and CPU-oracle references of the early-termination cases of the
reference-API compositing kernels (tests/test_gpu_composite.py runs them on
the device, tests/test_composite_cases_cpu.py checks without one that the
cases do what they claim).

Two families, everything numpy / the C oracle on the CPU, built once and
shared read-only:

  * train cases (composite_rays_train forward / backward): rays whose serial
    fp32 transmittance crosses T_thresh at a chosen sample on either side of
    the kernels' 64-sample chunk, rays that never cross, alpha = 0 and
    alpha = 1 rays, empty rays and the overflow rays march_rays_train leaves
    behind, in a shuffled ray table with permuted output rows;
  * loop cases (march_rays / composite_rays and the device-driven render
    loop): the reference's inference loop (renderer.py:384-420) over a
    synthetic field that is an exact function of the sample position, so the
    device and the oracle composite bit-identical inputs.
"""
import functools

import numpy as np

import oracle
import ray_cases
from helpers import box_bitfield, lego_rays

F32 = np.float32

# ------------------------------------------------------------------ train cases

LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
EPS = (1e-3, -1e-3, 1e-2, -1e-2)
VARIANTS = (1, 2, 3)            # N mod kCompWaves (4 rays per workgroup)
T_THRESHES = (1e-4, 1e-2)
# kinds of ray
CROSS, NEVER, ZERO, INF, BIG, EMPTY, OVERFLOW, PAD = range(8)


def crossings(length):
    """The engineered crossing samples k* that fit a ray of `length` samples."""
    ks = {0, 1, 62, 63, 64, 65, 126, 127, 128, length - 2, length - 1}
    return sorted(k for k in ks if 0 <= k < length)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def train_case(variant, T_thresh):
    """One ray set: dict of sigmas [M], rgbs [M, 3], deltas [M, 2], rays [N, 3]
    (shuffled rows, rays[:, 0] a permutation), per table row: kind, kstar, eps,
    valid (composited at all), and the output gradients, indexed like the
    outputs by rays[:, 0]."""
    rng = np.random.default_rng(1000 + variant)
    LT = -np.log(np.float64(F32(T_thresh)))
    specs = []  # (kind, length, kstar, eps)
    e = 0
    for length in LENGTHS:
        for k in crossings(length):
            specs.append((CROSS, length, k, EPS[e % 4]))
            e += 1
        specs.append((NEVER, length, -1, 0.0))
    specs += [(ZERO, 65, -1, 0.0), (ZERO, 130, -1, 0.0), (INF, 100, 40, 0.0), (BIG, 70, 64, 0.0)]
    specs += [(EMPTY, 0, -1, 0.0)] * 3
    n_fixed = len(specs) + 2  # + the two overflow rays
    specs += [(PAD, 30 + 7 * i, -1, 0.0) for i in range((variant - n_fixed) % 4)]
    sig, dl0, offs = [], [], []
    cur = 0
    for kind, length, k, eps in specs:
        offs.append(cur)
        d0 = rng.uniform(0.003, 0.01, length)
        if kind == CROSS:    # T after sample k* ~ T_thresh exp(-LT eps)
            sd = np.full(length, LT / (k + 1) * (1 + eps))
        elif kind == NEVER:  # total optical depth <= 0.75 LT
            sd = rng.uniform(0.5, 1.5, length) * (0.5 * LT / length)
        elif kind in (INF, BIG):
            sd = rng.uniform(0.5, 1.5, length) * (0.3 * LT / length)
        elif kind == PAD:
            sd = np.log1p(np.exp(rng.standard_normal(length))) * 10 * d0
        else:
            sd = np.zeros(length)
        s = (sd / d0).astype(F32)
        if kind == INF:
            s[k] = np.inf
        if kind == BIG:
            s[k] = 1e9
        sig.append(s)
        dl0.append(d0.astype(F32))
        cur += length
    # the overflow rays: A owns the last 30 rows and runs 10 past the end, B
    # starts past the end
    tail = 30
    sig.append((rng.uniform(0, 30, tail)).astype(F32))
    dl0.append(rng.uniform(0.003, 0.01, tail).astype(F32))
    M = cur + tail
    specs += [(OVERFLOW, 40, -1, 0.0), (OVERFLOW, 5, -1, 0.0)]
    offs += [M - tail, M + 10]
    N = len(specs)
    assert N % 4 == variant and M < 20000
    sigmas = np.concatenate(sig)
    d0 = np.concatenate(dl0)
    deltas = np.stack([d0, d0 * rng.uniform(0.5, 1.5, M).astype(F32)], -1).astype(F32)
    rgbs = rng.random((M, 3), dtype=F32)
    order = rng.permutation(N)       # the table's row order
    index = rng.permutation(N)       # the output row of each ray
    kind = np.array([s[0] for s in specs])[order]
    length = np.array([s[1] for s in specs])[order]
    rays = np.stack([index, np.array(offs)[order], length], -1).astype(np.int32)
    return _freeze(dict(
        variant=variant, T_thresh=float(T_thresh), M=M, N=N, sigmas=sigmas, rgbs=rgbs, deltas=deltas,
        rays=rays, kind=kind, kstar=np.array([s[2] for s in specs])[order],
        eps=np.array([s[3] for s in specs])[order],
        valid=(length > 0) & (rays[:, 1].astype(np.int64) + length <= M),
        gws=rng.standard_normal(N).astype(F32), gdepth=rng.standard_normal(N).astype(F32),
        gimage=rng.standard_normal((N, 3)).astype(F32)))


def oracle_backward_into(case, fwd, grad_sigmas, grad_rgbs):
    """The C oracle's backward writing into the given (pre-filled) buffers: like
    the reference it touches only the rows up to each ray's stop sample."""
    p = oracle._p
    ins = [np.ascontiguousarray(case[k], F32) for k in ("gws", "gdepth", "gimage", "sigmas", "rgbs", "deltas")]
    outs = [np.ascontiguousarray(a, F32) for a in fwd]
    rays = np.ascontiguousarray(case["rays"], np.int32)
    rc = oracle.lib().oracle_composite_rays_train_backward(
        *[p(a) for a in ins], p(rays), *[p(a) for a in outs], oracle._u(case["M"]), oracle._u(case["N"]),
        oracle._f(case["T_thresh"]), p(grad_sigmas), p(grad_rgbs))
    assert rc == 0


def last_written(grad_sigmas, grad_rgbs, rays, valid):
    """Per table row: the last sample (ray-relative) some buffer holds a
    non-sentinel value at, -1 if none; and whether every row up to it is
    written in both buffers."""
    M = grad_sigmas.shape[0]
    stop = np.full(rays.shape[0], -1)
    solid = np.ones(rays.shape[0], bool)
    for n, (_, off, cnt) in enumerate(rays):
        if not valid[n]:
            lo, hi = min(int(off), M), min(int(off) + int(cnt), M)
            solid[n] = np.isnan(grad_sigmas[lo:hi]).all() and np.isnan(grad_rgbs[lo:hi]).all()
            continue
        ws = ~np.isnan(grad_sigmas[off:off + cnt])
        wc = ~np.isnan(grad_rgbs[off:off + cnt]).all(1)
        w = ws | wc
        stop[n] = cnt - 1 - int(np.argmax(w[::-1])) if w.any() else -1
        k = stop[n] + 1
        solid[n] = ws[:k].all() and (~np.isnan(grad_rgbs[off:off + k])).all() and not (ws[k:].any() or wc[k:].any())
    return stop, solid


@functools.lru_cache(maxsize=None)
def train_reference(variant, T_thresh):
    """The oracle's forward, its backward over NaN-filled buffers, and the stop
    sample read off them."""
    c = train_case(variant, T_thresh)
    fwd = oracle.composite_rays_train_forward(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["T_thresh"])
    gs = np.full(c["M"], np.nan, F32)
    gc = np.full((c["M"], 3), np.nan, F32)
    oracle_backward_into(c, fwd, gs, gc)
    stop, solid = last_written(gs, gc, c["rays"], c["valid"])
    assert solid.all()
    return _freeze(dict(ws=fwd[0], depth=fwd[1], image=fwd[2], grad_sigmas=gs, grad_rgbs=gc, stop=stop))


def serial_stop(case):
    """fp32 restatement of the reference's recurrence (T *= 1 - alpha, break on
    T < T_thresh; raymarching.cu:540-557): per table row the stop sample (the
    last one when the ray never crosses), whether the break fired, and how
    close T came to T_thresh at the crossing (relative, the nearer of the last
    T above and the first below; inf when the ray never crosses)."""
    Tth = F32(case["T_thresh"])
    N = case["N"]
    stop = np.full(N, -1)
    fired = np.zeros(N, bool)
    margin = np.full(N, np.inf)
    sig, d0 = case["sigmas"], case["deltas"][:, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        for n, (_, off, cnt) in enumerate(case["rays"]):
            if not case["valid"][n]:
                continue
            T = F32(1)
            stop[n] = cnt - 1
            for s in range(cnt):
                alpha = F32(1) - np.exp(-sig[off + s] * d0[off + s], dtype=F32)
                Tp, T = T, F32(T * (F32(1) - alpha))
                if T < Tth:
                    stop[n], fired[n] = s, True
                    margin[n] = min(np.float64(Tp) / np.float64(Tth) - 1.0, 1.0 - np.float64(T) / np.float64(Tth))
                    break
    return stop, fired, margin


def float64_backward(case, stop):
    """torch-CPU float64 autograd of the plain compositing formula
    (w_i = alpha_i prod_{j<i} (1 - alpha_j), t_i = sum of the real deltas) over
    each ray's first stop + 1 samples: grad_sigmas [M], grad_rgbs [M, 3], zero
    outside those samples."""
    import torch
    rays, M = case["rays"], case["M"]
    rows = [np.arange(off, off + stop[n] + 1) for n, (_, off, _c) in enumerate(rays) if case["valid"][n]]
    idx = np.array([r[0] for n, r in enumerate(rays) if case["valid"][n]])
    L = max(len(r) for r in rows)
    R = len(rows)
    gather = np.zeros((R, L), np.int64)
    mask = np.zeros((R, L), bool)
    for i, r in enumerate(rows):
        gather[i, :len(r)], mask[i, :len(r)] = r, True
    m = torch.from_numpy(mask)
    sigma = torch.from_numpy(case["sigmas"].astype(np.float64)[gather]).masked_fill(~m, 0.0).requires_grad_(True)
    rgb = torch.from_numpy(case["rgbs"].astype(np.float64)[gather]).requires_grad_(True)
    d0 = torch.from_numpy(case["deltas"][:, 0].astype(np.float64)[gather]).masked_fill(~m, 0.0)
    d1 = torch.from_numpy(case["deltas"][:, 1].astype(np.float64)[gather]).masked_fill(~m, 0.0)
    sd = sigma * d0
    cs = torch.cumsum(sd, 1)
    T = torch.exp(-torch.cat([torch.zeros(R, 1, dtype=torch.float64), cs[:, :-1]], 1))
    w = (1 - torch.exp(-sd)) * T
    t = torch.cumsum(d1, 1)
    f = lambda k: torch.from_numpy(case[k].astype(np.float64)[idx])  # noqa: E731
    loss = (f("gws") * w.sum(1)).sum() + (f("gdepth") * (w * t).sum(1)).sum() + \
        (f("gimage") * (w[:, :, None] * rgb).sum(1)).sum()
    loss.backward()
    gs, gc = np.zeros(M), np.zeros((M, 3))
    gs[gather[mask]] = sigma.grad.numpy()[mask]
    gc[gather[mask]] = rgb.grad.numpy()[mask]
    live = np.zeros(M, bool)
    live[gather[mask]] = True
    return gs, gc, live


def float64_errors(grad_sigmas, grad_rgbs, ref):
    """(max |d grad_sigmas|, max over entries of |d| / (|ref| + 1e-3 max |ref|),
    max |d grad_rgbs|) over the rows the float64 reference covers."""
    gs, gc, live = ref
    ds = np.abs(grad_sigmas[live].astype(np.float64) - gs[live])
    dc = np.abs(grad_rgbs[live].astype(np.float64) - gc[live])
    return float(ds.max()), float((ds / (np.abs(gs[live]) + 1e-3 * np.abs(gs[live]).max())).max()), float(dc.max())


# ------------------------------------------------------------------- loop cases

# the occupied region of configurations (a) and (c): most Lego rays cross it
LOOP_BOXES = [((-0.75, -0.75, -0.6), (0.75, 0.75, 0.6))]
LOGITS = (np.arange(256) - 128) / 32.0   # the colour logits' alphabet (exact in fp16)
SIGMA_SOLID = 4000.0
SIGMA_RAMP = 150.0

LOOP_CONFIGS = {
    "a": dict(N=1024, bound=1.0, C=1, dt_gamma=0.0, T_thresh=1e-4, max_steps=1024, bits="box", seed=21, noise=False),
    "b": dict(N=1000, bound=2.0, C=2, dt_gamma=1 / 128, T_thresh=1e-2, max_steps=1024, bits="fox", seed=22, noise=True),
    "c": dict(N=1024, bound=1.0, C=1, dt_gamma=0.0, T_thresh=1e-4, max_steps=24, bits="box", seed=21, noise=False),
    # rays the Lego ring never produces (tests/ray_cases.py): cameras inside the box, exact zeros in
    # directions, NaN near or far, rays pointing away from the box and rays that miss it
    "d": dict(N=320, bound=2.0, C=2, dt_gamma=1 / 128, T_thresh=1e-2, max_steps=1024, bits="random", seed=23, noise=True,
              families=("interior", "axis", "face", "away", "miss"), min_near=0.05),
}
ALIVE, BY_T, RAN_OUT = 0, 1, 2
GRID_H = 128


def _cells(xyz):
    """Cell coordinates floor((xyz + 2) * 8) and the position inside the cell,
    in float32 (the subtraction is exact)."""
    p = (np.asarray(xyz, F32) + F32(2)) * F32(8)
    c = np.floor(p)
    return c.astype(np.int64), p - c


def _hash(xyz):
    c, _ = _cells(xyz)
    h =(c[:, 0] * 73856093) ^ (c[:, 1] * 19349663) ^ (c[:, 2] * 83492791)
    h &= 0xffffffff
    h ^= h >> 15
    h = (h * 0x2c1b3c6d) & 0xffffffff
    h ^= h >> 12
    h = (h * 0x297a2d39) & 0xffffffff
    h ^= h >> 15
    return h


def field(xyz):
    """sigma [M] float32 and colour logits [M, 3] float16, an exact function of
    the float32 position. By cell of floor((xyz + 2) * 8): empty (sigma 0),
    solid (SIGMA_SOLID: alpha = 1 to six digits), or a ramp across the cell
    from half to all of a per-cell peak <= SIGMA_RAMP (squared, so thin cells
    are common). The ramp keeps the equally spaced samples of a ray from
    giving expf the same argument dozens of times: over a constant cell one
    argument on which two expf differ in the last place moves weight_sum by
    6e-8 per sample, all the same way, and 17 samples of it are past the
    atol = 1e-6 the comparison inherits from random inputs."""
    h = _hash(xyz)
    cls = h % 16
    u = ((h >> 4) % 1024).astype(np.float64) / 1024.0
    along = 0.5 + _cells(xyz)[1].astype(np.float64).sum(1) / 6.0
    sigma = np.where(cls < 7, 0.0, np.where(cls == 15, SIGMA_SOLID, SIGMA_RAMP * u * u * along)).astype(F32)
    logits = np.stack([LOGITS[(h >> s) & 0xff] for s in (8, 16, 24)], -1).astype(np.float16)
    return sigma, logits


def sigmoid_h(logits):
    """torch.sigmoid of a half under autocast: fp32 math, half result, then the
    compositor's float cast."""
    x = np.asarray(logits, np.float16).astype(F32)
    return (F32(1) / (F32(1) + np.exp(-x, dtype=F32))).astype(np.float16).astype(F32)


@functools.lru_cache(maxsize=None)
def loop_inputs(name):
    from nerf.provider import fox_bitfield
    cfg = LOOP_CONFIGS[name]
    N, bound = cfg["N"], cfg["bound"]
    if "families" in cfg:  # the named ray families of tests/ray_cases.py, concatenated
        fams = ray_cases.families(bound, np.random.default_rng(cfg["seed"]))
        ro = np.concatenate([fams[f][0] for f in cfg["families"]])
        rd = np.concatenate([fams[f][1] for f in cfg["families"]])
        assert ro.shape[0] == N
    else:
        ro, rd = lego_rays(N, seed=cfg["seed"])
        if bound > 1:
            ro = ro * F32(bound / 2.0)
    aabb = np.array([-bound] * 3 + [bound] * 3, F32)
    nears, fars = oracle.near_far_from_aabb(ro, rd, aabb, cfg.get("min_near", 0.2))
    if cfg["bits"] == "fox":
        bits = fox_bitfield()
    elif cfg["bits"] == "random":  # 30 % of the cells of every cascade, at random
        bits = ray_cases.bitfield(cfg["C"], GRID_H, 0.3, cfg["seed"])
    else:
        bits = box_bitfield(LOOP_BOXES, cascade=cfg["C"], bound=bound, H=GRID_H)
    noises = np.random.default_rng(cfg["seed"] + 100).random(N, dtype=F32) if cfg["noise"] else np.zeros(N, F32)
    return _freeze(dict(cfg, name=name, rays_o=ro, rays_d=rd, aabb=aabb, nears=nears, fars=fars,
                        bits=np.ascontiguousarray(bits), noises=noises))


def _trail(inp, it, alive, rays_t, sig, rgb, deltas, ws, dp, img, book):
    """The same iteration one sample at a time through the C oracle (on
    copies): what ended each ray, and every T = 1 - weight_sum the oracle
    tested. Returns the copies for the caller to compare with the whole call."""
    n_alive, n_step = sig.shape[0] // it["n_step"], it["n_step"]
    Tth = np.float64(F32(inp["T_thresh"]))
    rt, w, d, im = rays_t.copy(), ws.copy(), dp.copy(), img.copy()
    s2, c3, d2 = sig.reshape(n_alive, n_step), rgb.reshape(n_alive, n_step, 3), deltas.reshape(n_alive, n_step, 2)
    rows = np.arange(n_alive)
    out_alive = alive.copy()
    for s in range(n_step):
        if rows.size == 0:
            break
        al = alive[rows].copy()
        ids = al.copy()
        proc = d2[rows, s, 0] != 0
        T = (F32(1) - w[ids]).astype(np.float64)
        book["near"][ids[proc & (np.abs(T / Tth - 1.0) <= 1e-4)]] = True
        book["samples"][ids[proc]] += 1
        oracle.composite_rays(rows.size, 1, al, rt, s2[rows, s], c3[rows, s], d2[rows, s], w, d, im,
                              inp["T_thresh"])
        died = al < 0
        book["cause"][ids[died & proc]] = BY_T
        book["cause"][ids[died & ~proc]] = RAN_OUT
        book["death_iter"][ids[died]] = it["iter"]
        out_alive[rows[died]] = -1
        rows = rows[~died]
    return out_alive, rt, w, d, im


@functools.lru_cache(maxsize=None)
def oracle_loop(name):
    """The reference's inference loop on the oracle: per iteration the record
    the device runs are compared with, the final per-ray outputs, what ended
    each ray, and the near-threshold rays (some tested T within 1e-4 relative
    of T_thresh)."""
    inp = loop_inputs(name)
    N = inp["N"]
    ws, dp, img = np.zeros(N, F32), np.zeros(N, F32), np.zeros((N, 3), F32)
    alive = np.arange(N, dtype=np.int32)
    rays_t = inp["nears"].copy()
    book = dict(near=np.zeros(N, bool), samples=np.zeros(N, np.int64), cause=np.full(N, ALIVE),
                death_iter=np.full(N, -1))
    iters, step = [], 0
    while step < inp["max_steps"]:
        n_alive = alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        noises = inp["noises"][:n_alive] if step == 0 else np.zeros(n_alive, F32)
        xyzs, _, deltas = oracle.march_rays(n_alive, n_step, alive, rays_t, inp["rays_o"], inp["rays_d"],
                                            inp["bound"], inp["bits"], inp["C"], GRID_H, inp["nears"],
                                            inp["fars"], noises, inp["dt_gamma"], inp["max_steps"])
        sig, logits = field(xyzs)
        rgb = sigmoid_h(logits)
        it = dict(iter=len(iters), step=step, n_alive=n_alive, n_step=n_step, alive=alive.copy(), xyzs=xyzs,
                  deltas=deltas)
        t_alive, t_rt, t_ws, t_dp, t_img = _trail(inp, it, alive, rays_t, sig, rgb, deltas, ws, dp, img, book)
        after = alive.copy()
        oracle.composite_rays(n_alive, n_step, after, rays_t, sig, rgb, deltas, ws, dp, img, inp["T_thresh"])
        # n_step composites of one sample are the composite of n_step samples
        assert np.array_equal(after, t_alive) and np.array_equal(ws, t_ws) and np.array_equal(img, t_img)
        assert np.array_equal(dp, t_dp) and np.array_equal(rays_t[after[after >= 0]], t_rt[after[after >= 0]])
        it.update(alive_after=after, rays_t=rays_t.copy(), weights_sum=ws.copy())
        iters.append(_freeze(it))
        alive = after[after >= 0]
        step += n_step
    return _freeze(dict(iters=tuple(iters), step=step, alive_end=alive, weights_sum=ws, depth=dp, image=img, **book))
