"""Rays the Lego ring never produces, and their CPU-oracle references, for the
ray set-up and marching kernels (tests/test_gpu_rays.py runs them on the
device, tests/test_ray_cases_cpu.py checks without one that the cases do what
they claim and that every marching loop over them ends).

Everything numpy / the C oracle on the CPU, built once and shared read-only.
A case is one row of CASES over all the ray families concatenated.
"""
import functools
import zlib

import numpy as np

import oracle

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
SQRT3 = 1.7320508075688772
TINY = (1e-8, -1e-20, 1e-39, -1e-45)   # the last two are denormal in float32
CHAIN_LIMIT = 4096                     # chain indices one wave's 64 segments of 64 cover


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dirs(rng, n):
    return _unit(rng.standard_normal((n, 3)))


def box_families(lo, hi, rng, n=64):
    """The families on the box [lo, hi] (float32-exact corners): dict of name ->
    (rays_o, rays_d) float32 [n, 3]. Directions are unit length after float64
    normalisation unless a family's point is the components themselves.

      interior  origin uniform in the middle 90 % of the box, random direction
      centre    origin uniform in +-0.5 whatever the box (the finest cascade's
                unit cube: the only rays that sample level 0 when the step
                length alone puts every t >= 1 on a coarser level)
      diag      origin within 3 % of the (-,-,-) corner, inside, direction along
                the diagonal + 5 % jitter: the longest chords
      axis      origin uniform in 1.5 x the box (inside and outside), direction
                +-e_k, the other two components a random mix of +0.0 and -0.0
      planar    interior origin, one direction component exactly 0
      tiny      interior origin, one direction component from TINY
      face      interior origin with one coordinate exactly on a face. Even
                rays: that axis' direction component is +0.0 or -0.0 (the
                slab's 0 * inf: NaN near on the low face, NaN far on the high
                face with +0.0; the miss marker with -0.0). Odd rays: a random
                direction turned into the box, every fourth of them out of it
      away      origin on the sphere of 3 x the largest half extent, pointing
                outward: near = min_near > far, no miss marker
      miss      the same origins, tangential directions: the slab test fails
      graze     origin 2.5 x a corner, aimed within 2e-3 of that corner: the
                three slabs' entry times nearly coincide, then the ray runs down
                the diagonal (or clips the corner, or misses)
    """
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    R = 3 * h.max()
    i = np.arange(n)
    k = i % 3

    def interior():
        return c + rng.uniform(-0.9, 0.9, (n, 3)) * h

    out = {}
    out["interior"] = (interior(), _dirs(rng, n))
    out["centre"] = (rng.uniform(-0.5, 0.5, (n, 3)), _dirs(rng, n))
    out["diag"] = (lo + rng.uniform(0, 0.03, (n, 3)) * h, _unit(h * (1 + 0.05 * rng.uniform(-1, 1, (n, 3)))))
    d = np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0)
    d[i, k] = np.where((i // 3) % 2 == 0, 1.0, -1.0)
    out["axis"] = (c + rng.uniform(-1.5, 1.5, (n, 3)) * h, d)
    d = _dirs(rng, n)
    d[i, k] = 0.0
    out["planar"] = (interior(), _unit(d))
    d = _dirs(rng, n)
    d[i, k] = 0.0
    d = _unit(d).astype(F32)
    d[i, k] = np.array(TINY)[(i // 3) % 4].astype(F32)
    out["tiny"] = (interior(), d)
    o = interior().astype(F32)
    high = (i // 2) % 2 == 1
    # (near and far start from the x slab, the only one whose NaN survives the comparisons:
    # half of the even rays sit on an x face)
    kf = np.where(i % 2 == 1, k, np.where((i // 8) % 2 == 0, 0, 1 + (i // 16) % 2))
    o[i, kf] = np.where(high, hi[kf], lo[kf]).astype(F32)
    d = _dirs(rng, n)
    inward = np.where(high, -1.0, 1.0) * np.abs(d[i, kf])
    d[i, kf] = np.where(i % 8 == 7, -inward, inward)
    d[i[::2], kf[::2]] = 0.0
    d = _unit(d)
    d[i[::2], kf[::2]] = np.where((i[::2] // 4) % 2 == 0, 0.0, -0.0)
    out["face"] = (o, d)
    u = _dirs(rng, n)
    out["away"] = (c + R * u, _unit(u + 0.01 * rng.standard_normal((n, 3))))
    u = _dirs(rng, n)
    out["miss"] = (c + R * u, _unit(np.cross(u, _dirs(rng, n))))
    s = np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
    o = c + 2.5 * s * h
    out["graze"] = (o, _unit(c + s * h + rng.uniform(-2e-3, 2e-3, (n, 3)) * h - o))
    return {name: (np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)) for name, (o, d) in out.items()}


def families(bound, rng, n=64):
    return box_families([-bound] * 3, [bound] * 3, rng, n)


FAMILIES = ("interior", "centre", "diag", "axis", "planar", "tiny", "face", "away", "miss", "graze")

# name -> (bound, C, dt_gamma, min_near, H, max_steps, occupancy density)
CASES = {
    "b1":        (1.0, 1, 0.0, 0.2, 128, 1024, 0.3),
    "b1.5":      (1.5, 2, 1 / 128, 0.05, 128, 1024, 0.3),
    "b2":        (2.0, 2, 1 / 128, 0.05, 128, 1024, 0.3),
    "b2-h64":    (2.0, 2, 0.0, 0.0, 64, 1024, 0.3),
    "b3":        (3.0, 3, 1 / 256, 0.2, 128, 1024, 0.3),
    "b8":        (8.0, 4, 0.0, 0.2, 128, 1024, 0.3),         # OccGlobal; dt_gamma == 0 chains past CHAIN_LIMIT
    "b16":       (16.0, 5, 1 / 64, 0.05, 128, 1024, 0.3),    # dt_min, linear and dt_max on one ray
    "b16-long":  (16.0, 5, 1 / 1024, 0.05, 128, 4096, 0.3),  # ChainGamma chains past CHAIN_LIMIT
    "b2-full":   (2.0, 2, 0.0, 0.05, 128, 1024, 1.0),        # every index occupied: rays stop at max_steps
    # dt_min = 2 sqrt(3) / 1542 ends in nine zero bits, so in the binade [2, 4) dt_min / ulp(t) ends in
    # exactly .5: every step there is a round-to-even tie, and the step from a t with an odd last bit
    # is one ulp off the steps that follow it
    # (2 sqrt(3) / 2^k has an odd mantissa: a tie only where a binade holds two steps)
    "b2-ties":   (2.0, 2, 0.0, 0.05, 128, 1542, 0.3),
}
TIE_CASE, TIE_BINADE = "b2-ties", (2.0, 4.0)
CUT_CASE = "b1.5"     # also marched into a capacity that cuts the tail (reference(CUT_CASE, cut=True))
CUT_FRACTION = 0.6
# the interior rays of this case are also marched with these max_steps: dt_min > dt_max
SHORT_CASE, SHORT_MAX_STEPS = "b2", (1, 7)
# a non-cubic, off-centre box for the near / far kernels alone
OFF_AABB = (-1.5, -0.5, -1.0, 0.5, 1.25, 2.0)
OFF_MIN_NEAR = 0.05


@functools.lru_cache(maxsize=None)
def bitfield(C, H, density, seed):
    rng = np.random.default_rng(seed)
    bits = np.packbits(rng.random(C * H ** 3) < density, bitorder="little")
    bits.setflags(write=False)
    return bits


def march_consts(c):
    """dt_min, dt_max in float32 as the kernels form them."""
    dt_min = F32(2) * F32(SQRT3) / F32(c["max_steps"])
    dt_max = F32(2) * F32(SQRT3) * F32(1 << (c["C"] - 1)) / F32(c["H"])
    return dt_min, dt_max


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case: rays (all families, `slices` says where each
    sits), noises, the bitfield and the march constants."""
    bound, C, dt_gamma, min_near, H, max_steps, density = CASES[name]
    seed = zlib.crc32(name.encode())  # (of the name alone: a new row leaves the others as they are)
    rng = np.random.default_rng(seed)
    fams = families(bound, rng)
    assert tuple(fams) == FAMILIES
    slices, at = {}, 0
    for f in FAMILIES:
        slices[f] = slice(at, at + fams[f][0].shape[0])
        at = slices[f].stop
    ro = np.concatenate([fams[f][0] for f in FAMILIES])
    rd = np.concatenate([fams[f][1] for f in FAMILIES])
    return _freeze(dict(name=name, bound=bound, C=C, dt_gamma=dt_gamma, min_near=min_near, H=H, max_steps=max_steps,
                        density=density, N=at, slices=slices, rays_o=ro, rays_d=rd,
                        aabb=np.array([-bound] * 3 + [bound] * 3, F32), noises=rng.random(at, dtype=F32),
                        bits=bitfield(C, H, density, seed)))


def _march(c, ro, rd, nears, fars, noises, M, counter, max_steps=None):
    return oracle.march_rays_train(ro, rd, c["bound"], c["bits"], c["C"], c["H"], nears, fars, noises, M=M,
                                   dt_gamma=c["dt_gamma"], max_steps=max_steps or c["max_steps"], counter=counter)


@functools.lru_cache(maxsize=None)
def reference(name, cut=False, counter0=0):
    """The oracle's near_far_from_aabb and march_rays_train of a case, with the
    per-ray noises it marched with. M is the
    sample total + 64 (so nothing is dropped), or with cut=True CUT_FRACTION of
    the total (the oracle leaves the rays past it without rows); counter0 is
    the sample offset the march starts from."""
    c = case(name)
    nears, fars = oracle.near_far_from_aabb(c["rays_o"], c["rays_d"], c["aabb"], c["min_near"])
    args = (c, c["rays_o"], c["rays_d"], nears, fars, c["noises"])
    total = int(_march(*args, M=0, counter=(0, 0))[3][:, 2].sum())
    M = int(total * CUT_FRACTION) if cut else counter0 + total + 64
    xyzs, dirs, deltas, rays, counter = _march(*args, M=M, counter=(counter0, 3))
    return _freeze(dict(nears=nears, fars=fars, noises=c["noises"], M=M, total=total, xyzs=xyzs, dirs=dirs,
                        deltas=deltas, rays=rays, counter=counter))


@functools.lru_cache(maxsize=None)
def short_reference(max_steps):
    """The interior rays of SHORT_CASE marched with a max_steps so small that
    dt_min > dt_max (clampf's argument order decides the step)."""
    c, r = case(SHORT_CASE), reference(SHORT_CASE)
    s = c["slices"]["interior"]
    ins = dict(rays_o=c["rays_o"][s], rays_d=c["rays_d"][s], nears=r["nears"][s], fars=r["fars"][s],
               noises=c["noises"][s])
    N = s.stop - s.start
    M = N * max_steps
    xyzs, dirs, deltas, rays, counter = _march(c, ins["rays_o"], ins["rays_d"], ins["nears"], ins["fars"],
                                               ins["noises"], M=M, counter=(0, 0), max_steps=max_steps)
    return _freeze(dict(ins, N=N, M=M, max_steps=max_steps, xyzs=xyzs, dirs=dirs, deltas=deltas, rays=rays,
                        counter=counter))


@functools.lru_cache(maxsize=None)
def off_centre():
    """All families on the OFF_AABB box, and the oracle's near / far."""
    lo, hi = OFF_AABB[:3], OFF_AABB[3:]
    fams = box_families(lo, hi, np.random.default_rng(77))
    ro = np.concatenate([fams[f][0] for f in FAMILIES])
    rd = np.concatenate([fams[f][1] for f in FAMILIES])
    aabb = np.array(OFF_AABB, F32)
    nears, fars = oracle.near_far_from_aabb(ro, rd, aabb, OFF_MIN_NEAR)
    return _freeze(dict(rays_o=ro, rays_d=rd, aabb=aabb, min_near=OFF_MIN_NEAR, nears=nears, fars=fars))


# ------------------------------------------------------------ what a case holds

def ray_t0(c, nears):
    """The first t of every ray's chain, in float32 as the kernels form it
    (fmaf(clamp(near * dt_gamma), noise, near): the product is exact in
    float64, one rounding)."""
    dt_min, dt_max = march_consts(c)
    with np.errstate(invalid="ignore", over="ignore"):
        dt0 = np.minimum(dt_max, np.maximum(dt_min, nears * F32(c["dt_gamma"])))
        return (dt0.astype(np.float64) * c["noises"].astype(np.float64) + nears.astype(np.float64)).astype(F32)


def chain_lengths(c, nears, fars, limit=4 * CHAIN_LIMIT):
    """Per ray the number of chain indices below far, t_{k+1} = t_k + clamp(t_k
    dt_gamma, dt_min, dt_max) stepped in float32 from t0 (0 for a ray that
    never starts; capped at `limit`)."""
    dt_min, dt_max = march_consts(c)
    g = F32(c["dt_gamma"])
    t = ray_t0(c, nears)
    K = np.zeros(t.shape[0], np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(limit):
            live = t < fars
            if not live.any():
                break
            K += live
            t = np.where(live, t + np.minimum(dt_max, np.maximum(dt_min, t * g)), t)
    return K


def sample_levels(c, xyzs, deltas):
    """The cascade level of every sample (mip_from_pos / mip_from_dt)."""
    def lvl(m):
        e = np.frexp(m.astype(F32))[1]
        return np.clip(np.where(m == 0, 0, e), 0, c["C"] - 1)
    return np.maximum(lvl(np.abs(xyzs).max(1)), lvl(deltas[:, 0] * F32(c["H"]) * F32(0.5)))


def box_distance(ro, aabb):
    """Distance from each origin to the box (0 inside), float64."""
    o = ro.astype(np.float64)
    lo, hi = aabb[:3].astype(np.float64), aabb[3:].astype(np.float64)
    return np.linalg.norm(np.maximum(np.maximum(lo - o, o - hi), 0.0), axis=1)


def termination_check(name):
    """What is argued before a case reaches a marching loop on the device:

      * every far is finite, the miss marker or NaN, never +inf; a finite far is
        at most 2 sqrt(3) bound (1 + 1e-3) past the distance from the origin to
        the box (for an origin inside: the box diagonal);
      * t + dt > t wherever a chain can reach. A loop runs while t < far and one
        DDA skip ends within 2 sqrt(3) bound + dt_max of where it began, so t <=
        t_max = far_max + 2 sqrt(3) bound + dt_max. The step at t is clamp(t
        dt_gamma, dt_min, dt_max) and ulp(t) <= 2^-23 t: while the step is dt_min
        or linear in t it is >= dt_gamma 2^23 ulps of t (dt_gamma > 0), at dt_max
        (or with dt_gamma == 0) >= step / ulp(t_max). Both must be >= 2^8; half
        an ulp is what progress needs. (2^10 against dt_min alone cannot hold
        for the (16, 5, 1/64) and (16, 5, 1/1024) rows: dt_min 3.4e-3 / 8.5e-4
        against 2^10 ulp(55) = 3.9e-3; there the step at t = 55 is 0.43 / 0.054.)

    Returns the margin in ulps."""
    c, r = case(name), reference(name)
    fars, bound = r["fars"], c["bound"]
    assert not np.isposinf(fars).any() and not np.isinf(r["nears"]).any()
    fin = np.isfinite(fars) & (fars != FLT_MAX)
    assert (np.isnan(fars) | (fars == FLT_MAX) | fin).all()
    cap = 2 * SQRT3 * bound * (1 + 1e-3) + box_distance(c["rays_o"], c["aabb"])
    assert (fars[fin] <= cap[fin]).all(), float((fars[fin] - cap[fin]).max())
    dt_min, dt_max = march_consts(c)
    t_max = F32(max(float(fars[fin].max()), 0.0) + 2 * SQRT3 * bound + float(dt_max))
    flat = float(dt_max if c["dt_gamma"] > 0 else np.minimum(dt_max, np.maximum(dt_min, F32(0))))
    margin = flat / float(np.spacing(t_max))
    if c["dt_gamma"] > 0:
        margin = min(margin, c["dt_gamma"] * 2.0 ** 23)
    assert margin >= 2 ** 8, margin
    return margin


def summary(name):
    """One line per case for the parity summary."""
    c, r = case(name), reference(name)
    K = chain_lengths(c, r["nears"], r["fars"])
    n = r["rays"][:, 2]
    return (f"{name}: {c['N']} rays, {r['total']} samples, {int((n > 0).sum())} rays sampled, "
            f"{int((np.isnan(r['nears']) | np.isnan(r['fars'])).sum())} NaN, {int((r['fars'] == FLT_MAX).sum())} miss, "
            f"{int((K > CHAIN_LIMIT).sum())} long-chain, {int((n == c['max_steps']).sum())} capped")
