"""The cases of the background backward's entry-level tests
(tests/test_gpu_background_backward.py runs them on the kernel,
tests/test_background_cases_cpu.py proves their conditions on the CPU): the
grids that take each route of k_bg_backward, the ray counts and rays lists, and
seeded inputs on which the float64 reference's ReLU mask is certain.

No product imports: the level offsets are restated from GridEncoder's rule and
the GPU test asserts they are the encoder's own."""
import functools
from collections import namedtuple

import numpy as np

import background_helpers as bh

RADIUS = 3.0
SCALE = 128.0
LVL0_MAX = 1024         # kLvl0Max: level 0's values a workgroup sums in LDS
ONE_PASS = 64 * 256     # kMaxBwdBlocks * kBwdThreads: more rays take a second loop pass
DESIRED = 2048

# rays: None (identity order), "perm" (a seeded permutation), "holes" (a
# permutation whose every 5th entry is -1 or N + 3). live: the rays that carry
# gradient, "all" or "tail" (out_ws = 1 exactly below ONE_PASS).
Case = namedtuple("Case", "name N base log2T rays live color_weight seed")
CASES = [Case("default", 257, 16, 19, "perm", "all", 1.0, 1)]
CASES += [Case(f"ragged{n}", n, 16, 19, None, "all", 1.0, 10 + k) for k, n in enumerate((1, 63, 64, 65, 255))]
CASES += [Case("level0_global", 257, 32, 19, "perm", "all", 1.0, 2),
          Case("level0_hashed", 257, 16, 8, "perm", "all", 1.0, 3),
          Case("second_pass", ONE_PASS + 65, 16, 19, None, "tail", 1.0, 4),
          Case("second_pass_all", ONE_PASS + 65, 16, 19, None, "all", 1.0, 5),
          Case("holes", 257, 16, 19, "holes", "all", 1.0, 6),
          Case("named_rays", 65, 16, 19, None, "all", 0.5, 7)]
BY_NAME = {c.name: c for c in CASES}
FORWARD_CASES = ["named_rays", "level0_global", "level0_hashed"]


def grid_spec(base, log2T, desired=DESIRED):
    """GridEncoder(input_dim=2, num_levels=4, level_dim=2, base_resolution=base,
    log2_hashmap_size=log2T, desired_resolution=desired): (offsets, S =
    log2(per_level_scale))."""
    pls = np.exp2(np.log2(desired / base) / 3)
    offsets, offset = [], 0
    for i in range(4):
        res = int(np.ceil(base * pls ** i))
        n = min(2 ** log2T, (res + 1) ** 2)
        offsets.append(offset)
        offset += int(np.ceil(n / 8) * 8)
    return offsets + [offset], float(np.log2(pls))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere_point(theta, phi):
    return RADIUS * np.array([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)])


def named_rays():
    """(names, o [K, 3], d [K, 3]) in float32, every origin inside the sphere:
    directions +-y (from a point on the axis: the poles themselves, where
    atan2(0, 0) decides phi, and from a point off it), directions (-1, 0, +-0)
    in the plane z = +-0 (phi = +-pi: the seam, x1 = 1 and 0), rays from the
    centre, and hit points 1e-3 rad on either side of the seam and of each pole."""
    rows = [("+y on the axis", (0, 0.5, 0), (0, 1, 0)), ("-y on the axis", (0, 0.5, 0), (0, -1, 0)),
            ("+y off the axis", (0.3, 0.1, -0.2), (0, 1, 0)), ("-y off the axis", (0.3, 0.1, -0.2), (0, -1, 0)),
            ("seam +0", (0.5, 0.2, 0.0), (-1, 0, 0.0)), ("seam -0", (0.5, 0.2, -0.0), (-1, 0, -0.0)),
            ("centre +y", (0, 0, 0), (0, 1, 0)), ("centre -y", (0, 0, 0), (0, -1, 0)),
            ("centre -x", (0, 0, 0), (-1, 0, 0.0)), ("centre -x -0", (0, 0, -0.0), (-1, 0, -0.0)),
            ("centre", (0, 0, 0), tuple(_unit(np.array([0.3, -0.5, 0.8])))),
            ("centre +x", (0, 0, 0), (1, 0, 0))]
    o_in = np.array([0.4, -0.3, 0.2])
    hits = [("seam + 1e-3", 1.0, -np.pi + 1e-3), ("seam - 1e-3", 1.0, np.pi - 1e-3),
            ("north pole, phi 0.7", 1e-3, 0.7), ("north pole, phi 0.7 - pi", 1e-3, 0.7 - np.pi),
            ("south pole, phi 0.7", np.pi - 1e-3, 0.7), ("south pole, phi 0.7 - pi", np.pi - 1e-3, 0.7 - np.pi)]
    for name, theta, phi in hits:
        rows.append((name, tuple(o_in), tuple(_unit(_sphere_point(theta, phi) - o_in))))
    names = [r[0] for r in rows]
    o = np.array([r[1] for r in rows], dtype=np.float32)
    d = np.array([r[2] for r in rows], dtype=np.float32)
    return names, o, d


def _draw_rays(rng, n):
    """Origins uniform in a ball of radius 2.4, unit directions (float32)."""
    o = _unit(rng.standard_normal((n, 3))) * 2.4 * rng.random((n, 1)) ** (1 / 3)
    return o.astype(np.float32), _unit(rng.standard_normal((n, 3))).astype(np.float32)


def _features(d):
    return bh.features64(d["o"], d["d"], RADIUS, d["table"], d["offsets"], d["base"], d["S"])


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The case's inputs, read-only numpy arrays: o, d [N, 3] float32; table
    [entries, 2] ~ N(0, 0.3) and weights [3072] ~ 4 x U(+-sqrt(3 / 64)) in fp16;
    out_image [N, 3], gt [N, 4], out_ws [N] uniform float32; rays [N, 3] int32 or
    None; offsets, base, S; `redrawn`, the rays drawn again because a hidden
    unit's mask was not certain (bh.uncertain_units on the float64 features,
    rounded to half), and `fixed`, the leading rays that are never redrawn."""
    case = BY_NAME[name]
    N = case.N
    rng = np.random.default_rng(1000 + case.seed)
    offsets, S = grid_spec(case.base, case.log2T)
    d = dict(offsets=offsets, base=case.base, S=S, N=N)
    d["table"] = (rng.standard_normal((offsets[-1], 2)) * 0.3).astype(np.float16)
    std = 4 * (3 / 64) ** 0.5
    d["weights"] = rng.uniform(-std, std, 64 * (32 + 16)).astype(np.float16)
    d["o"], d["d"] = _draw_rays(rng, N)
    fixed = 0
    if name == "named_rays":
        _, o, dd = named_rays()
        fixed = o.shape[0]
        d["o"][:fixed], d["d"][:fixed] = o, dd
    d["out_image"] = rng.random((N, 3), dtype=np.float32)
    d["gt"] = rng.random((N, 4), dtype=np.float32)
    d["out_ws"] = rng.random(N, dtype=np.float32)
    if case.live == "tail":
        d["out_ws"][:ONE_PASS] = 1.0
    if case.rays is None:
        d["rays"] = None
    else:
        order = rng.permutation(N).astype(np.int32)
        if case.rays == "holes":
            order[0::10], order[5::10] = -1, N + 3
        rays = rng.integers(0, 1 << 20, (N, 3)).astype(np.int32)  # (columns 1, 2: the sample offset and count, not read)
        rays[:, 0] = order
        d["rays"] = rays
    # the certain ReLU mask: redraw the rays with a unit too close to zero
    redrawn = np.zeros(N, dtype=bool)
    for _ in range(8):
        x = _features(d).astype(np.float16)
        bad = np.flatnonzero(bh.uncertain_units(x, d["weights"]).any(1))
        bad = bad[bad >= fixed]
        if bad.size == 0:
            break
        redrawn[bad] = True
        d["o"][bad], d["d"][bad] = _draw_rays(rng, bad.size)
    else:
        raise AssertionError(f"{name}: the mask did not become certain")
    d["redrawn"], d["fixed"] = int(redrawn.sum()), fixed
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def cpu_saved(d, exact=False):
    """What the forward would keep, from the float64 model (the CPU tests' stand-
    in for the kernel's x_save, sph_save and bg): x [N, 32] rounded to half,
    sph01 [N, 2] and bg [N, 3] in float32; exact: all three left in float64."""
    x = _features(d)
    sph01 = (bh.sph64(d["o"], d["d"], RADIUS) + 1) / 2
    if exact:
        return x, sph01, bh.mlp64(x, d["weights"])
    x = x.astype(np.float16)
    return x, sph01.astype(np.float32), bh.mlp64(x.astype(np.float64), d["weights"]).astype(np.float32)


def order_of(d):
    return None if d["rays"] is None else d["rays"][:, 0]
