"""numpy restatement of the error-map sampler (include/ngp_hip.h:
ngp_error_map_select, ngp_image_source's error_map fields, ngp_error_map_update),
written from its formulas: the counter RNG, the exponential-race keys, the
top-N selection under the tie rule, the ray permutation, the cell -> pixel
rule and the EMA, the fp32 parts in np.float32 operations."""
import math

import numpy as np

ALL = 0xFFFFFFFF
M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & M32


def mix32(x):
    x = _u64(x)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def rng_u32(seed, a, b, c):
    """mix32(seed ^ mix32(a + 0x9e3779b9 * mix32(b ^ mix32(c + 0x85ebca6b)))), all mod 2^32."""
    inner = mix32((_u64(c) + np.uint64(0x85EBCA6B)) & M32)
    mid = mix32(_u64(b) ^ inner)
    outer = mix32((_u64(a) + ((np.uint64(0x9E3779B9) * mid) & M32)) & M32)
    return mix32(_u64(seed) ^ outer)


def rng_unit(seed, a, b, c):
    """(float)(rng >> 8) * 2^-24 in fp32 (both factors exact, so is the product)."""
    return (rng_u32(seed, a, b, c) >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def pose_of(seed, it, n_poses):
    return int(rng_u32(seed, it, ALL, 0)) % n_poses


def keys64(w, seed, it):
    """The race's keys in float64: w / -log((k + 1) * 2^-24), 0 for w <= 0."""
    w = np.asarray(w, dtype=np.float64)
    c = np.arange(w.size, dtype=np.uint64)
    k = rng_u32(seed, it, c, 6) >> np.uint64(8)
    u = (k.astype(np.float64) + 1.0) * 2.0 ** -24
    with np.errstate(divide="ignore"):
        key = w / -np.log(u)  # u = 1: w / 0 = +inf
    return np.where(w > 0, np.abs(key), 0.0)


def top_n(keys, n):
    """The n cells with the largest keys, ties to the lower cell; ascending."""
    keys = np.asarray(keys)
    order = np.argsort(-keys.astype(np.float64), kind="stable")  # stable: equal keys keep cell order
    return np.sort(order[:n]).astype(np.int64)


def perm_mult(n):
    """The largest integer <= 0.618 n coprime to n, at least 1."""
    p = int(0.618 * n)
    while p > 1 and math.gcd(p, n) != 1:
        p -= 1
    return max(p, 1)


def coarse_of(selected, seed, it):
    """Ray i's cell: selected[(i * perm_mult + r) % N], r = rng_u32(seed, it, ALL, 1) % N."""
    selected = np.asarray(selected, dtype=np.int64)
    n = selected.size
    r = int(rng_u32(seed, it, ALL, 1)) % n
    rank = (np.arange(n, dtype=np.int64) * perm_mult(n) + r) % n
    return selected[rank]


def pix_of(coarse, H, W, res, seed, it):
    """row = min((uint32)((float)(cell / res) * sx + u7 * sx), H - 1), col likewise with
    cell % res, sy, stream 8 and W - 1; pix = row * W + col. fp32, no contraction."""
    coarse = np.asarray(coarse, dtype=np.int64)
    n = np.arange(coarse.size, dtype=np.uint64)
    sx, sy = np.float32(H) / np.float32(res), np.float32(W) / np.float32(res)
    fx = (coarse // res).astype(np.float32) * sx + rng_unit(seed, it, n, 7) * sx
    fy = (coarse % res).astype(np.float32) * sy + rng_unit(seed, it, n, 8) * sy
    assert fx.dtype == np.float32 and fy.dtype == np.float32
    row = np.minimum(fx.astype(np.int64), H - 1)
    col = np.minimum(fy.astype(np.int64), W - 1)
    return row * W + col


def colour_err(out_image, rgba, bg):
    """((e0^2 + e1^2) + e2^2) * (1/3)f with e = image - (rgb * a + bg * (1 - a)), per row, fp32."""
    out_image, rgba, bg = (np.asarray(t, dtype=np.float32) for t in (out_image, rgba, bg))
    a = rgba[:, 3:4]
    q = rgba[:, :3] * a + bg * (np.float32(1.0) - a)
    e = out_image - q
    s = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return s * (np.float32(1.0) / np.float32(3.0))


def ema(old, err):
    """0.1f * old + 0.9f * err in fp32."""
    return np.float32(0.1) * np.asarray(old, np.float32) + np.float32(0.9) * np.asarray(err, np.float32)


def inclusion_counts(res, n, draws, seed):
    """Per-cell inclusion counts of `draws` uniform-weight selections (the CPU oracle)."""
    counts = np.zeros(res * res, dtype=np.int64)
    w = np.ones(res * res)
    for it in range(draws):
        counts[top_n(keys64(w, seed, it), n)] += 1
    return counts
