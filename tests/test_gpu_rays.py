"""GPU: ray set-up and marching on rays the Lego ring never produces, against
the CPU oracle (cases: tests/ray_cases.py, checked without a GPU in
tests/test_ray_cases_cpu.py): cameras inside the box, exact / negative zeros
and denormals in directions, NaN near or far, rays that miss or point away,
every binade from min_near up, the three dt regimes on one ray, chains past
the wave's 4096 indices, four and five cascades, non-power-of-two bounds.

Everything is compared bit for bit. The one exception is NaN: where the
oracle has a NaN the device must have one, and its payload is not compared
(0 * inf carries the sign bit on x86 and need not on the device).
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import ray_cases as rc

pytestmark = pytest.mark.gpu

NAMES = sorted(rc.CASES)


@pytest.fixture(scope="module", autouse=True)
def loops_end():
    """No case reaches a marching kernel before the termination argument has
    been checked for it on the CPU (tests/test_ray_cases_cpu.py asserts the
    same per case)."""
    for name in NAMES:
        rc.termination_check(name)


def t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a copy: the cases are read-only)


def assert_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions", np.flatnonzero(np.isnan(got) != nan)[:8])
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], ref[bad][:4])


def _near_far(cuda, ro, rd, aabb, min_near):
    import raymarching.backend as rb
    N = ro.shape[0]
    nears, fars = torch.full((N,), -7.0, device=cuda), torch.full((N,), -7.0, device=cuda)
    rb._backend.near_far_from_aabb(t(ro, cuda), t(rd, cuda), t(aabb, cuda), N, min_near, nears, fars)
    return nears.cpu().numpy(), fars.cpu().numpy()


@pytest.mark.parametrize("name", NAMES + ["off-centre"])
def test_near_far(cuda, name):
    if name == "off-centre":
        c = r = rc.off_centre()
    else:
        c, r = rc.case(name), rc.reference(name)
    nears, fars = _near_far(cuda, c["rays_o"], c["rays_d"], c["aabb"], c["min_near"])
    assert_bits(nears, r["nears"], "nears")
    assert_bits(fars, r["fars"], "fars")


def _march_train(cuda, c, ins, M, max_steps, counter):
    import raymarching.backend as rb
    N = ins["rays_o"].shape[0]
    xyzs, dirs, deltas = torch.zeros(M, 3, device=cuda), torch.zeros(M, 3, device=cuda), torch.zeros(M, 2, device=cuda)
    rays = torch.full((N, 3), -7, dtype=torch.int32, device=cuda)
    cnt = t(np.array(counter, np.int32), cuda)
    rb._backend.march_rays_train(t(ins["rays_o"], cuda), t(ins["rays_d"], cuda), t(c["bits"], cuda), c["bound"],
                                 c["dt_gamma"], max_steps, N, c["C"], c["H"], M, t(ins["nears"], cuda),
                                 t(ins["fars"], cuda), xyzs, dirs, deltas, rays, cnt, t(ins["noises"], cuda))
    return [a.cpu().numpy() for a in (xyzs, dirs, deltas, rays, cnt)]


def _check_march(got, again, r, rows):
    xyzs, dirs, deltas, rays, counter = got
    assert np.array_equal(rays, r["rays"]), np.flatnonzero((rays != r["rays"]).any(1))[:8]
    assert np.array_equal(counter, r["counter"])
    for g, name in ((xyzs, "xyzs"), (dirs, "dirs"), (deltas, "deltas")):
        assert_bits(g[:rows], r[name][:rows], name)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))  # the same bits on every run


MARCH = [(n, False, 0) for n in NAMES] + [(rc.CUT_CASE, True, 0), ("b1", False, 1000)]


@pytest.mark.parametrize("name,cut,counter0", MARCH, ids=[n + ("-cut" if c else "") + (f"-from{k}" if k else "")
                                                        for n, c, k in MARCH])
def test_march_rays_train(cuda, parity_report, name, cut, counter0):
    """_backend.march_rays_train on every case: rays, counter and the rows of
    xyzs / dirs / deltas up to counter[0]; with a capacity that cuts the tail
    the whole buffers (the dropped rays' rows stay zero); from a non-zero
    counter the rows before it stay zero too. The nears / fars are the
    oracle's, NaN included."""
    c, r = rc.case(name), rc.reference(name, cut=cut, counter0=counter0)
    ins = dict(rays_o=c["rays_o"], rays_d=c["rays_d"], nears=r["nears"], fars=r["fars"], noises=c["noises"])
    runs = [_march_train(cuda, c, ins, r["M"], c["max_steps"], (counter0, 3)) for _ in range(2)]
    _check_march(runs[0], runs[1], r, r["M"] if cut or counter0 else int(r["counter"][0]))
    if not cut and not counter0:
        parity_report(rc.summary(name))


@pytest.mark.parametrize("max_steps", rc.SHORT_MAX_STEPS)
def test_march_rays_train_dt_min_above_dt_max(cuda, max_steps):
    """max_steps so small that dt_min > dt_max: clampf's argument order decides
    the step (fminf(hi, fmaxf(lo, x)) gives dt_max)."""
    c, r = rc.case(rc.SHORT_CASE), rc.short_reference(max_steps)
    runs = [_march_train(cuda, c, r, r["M"], max_steps, (0, 0)) for _ in range(2)]
    _check_march(runs[0], runs[1], r, r["M"])


def _march_rays(cuda, c, r, n_step, alive, rays_t, noises):
    import raymarching.backend as rb
    n_alive = alive.shape[0]
    Mi = n_alive * n_step
    xyzs, dirs, deltas = (torch.zeros(Mi, 3, device=cuda), torch.zeros(Mi, 3, device=cuda),
                          torch.zeros(Mi, 2, device=cuda))
    rb._backend.march_rays(n_alive, n_step, t(alive, cuda), t(rays_t, cuda), t(c["rays_o"], cuda), t(c["rays_d"], cuda),
                           c["bound"], c["dt_gamma"], c["max_steps"], c["C"], c["H"], t(c["bits"], cuda),
                           t(r["nears"], cuda), t(r["fars"], cuda), xyzs, dirs, deltas, t(noises, cuda))
    ref = oracle.march_rays(n_alive, n_step, alive, rays_t, c["rays_o"], c["rays_d"], c["bound"], c["bits"], c["C"],
                            c["H"], r["nears"], r["fars"], noises, c["dt_gamma"], c["max_steps"])
    for g, o, name in zip((xyzs, dirs, deltas), ref, ("xyzs", "dirs", "deltas")):
        assert_bits(g.cpu().numpy(), o, name)
    return ref


@pytest.mark.parametrize("n_step", [1, 8])
@pytest.mark.parametrize("name", NAMES)
def test_march_rays(cuda, name, n_step):
    """_backend.march_rays from rays_t = nears over a shuffled alive list that
    holds the away, miss and NaN rays too, then again from the rays_t and the
    alive list a composite of that round leaves (sigma = 0: every ray that
    filled its n_step stays alive at t advanced by its deltas)."""
    c, r = rc.case(name), rc.reference(name)
    N = c["N"]
    rng = np.random.default_rng(n_step)
    alive = rng.permutation(N)[:N - 37].astype(np.int32)
    dead = np.isnan(r["nears"]) | np.isnan(r["fars"]) | (r["fars"] == rc.FLT_MAX) | (r["fars"] < r["nears"])
    assert dead[alive].sum() >= 100
    rays_t = r["nears"].copy()
    xyzs, dirs, deltas = _march_rays(cuda, c, r, n_step, alive, rays_t, rng.random(alive.shape[0], dtype=np.float32))
    filled = (deltas.reshape(-1, n_step, 2)[:, :, 0] != 0).all(1)
    assert not filled[dead[alive]].any() and filled.sum() >= 100
    z = np.zeros(N, np.float32)
    after = alive.copy()
    oracle.composite_rays(alive.shape[0], n_step, after, rays_t, np.zeros(alive.shape[0] * n_step, np.float32),
                          np.zeros((alive.shape[0] * n_step, 3), np.float32), deltas, z.copy(), z.copy(),
                          np.zeros((N, 3), np.float32), 1e-4)
    assert np.array_equal(after >= 0, filled)
    moved = after[after >= 0]
    assert (rays_t[moved] > r["nears"][moved]).all()
    _march_rays(cuda, c, r, n_step, moved, rays_t, np.zeros(moved.shape[0], np.float32))


# ---- the second slab test: ngp_head::near_far in the frame and training-draw heads ----

HW = 8
INTR = (30.0, 20.0, 3.5, 4.5)   # fx != fy; column 3 has xs = 0 and row 4 ys = 0 exactly
HEAD_AABB = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
HEAD_MIN_NEAR = 0.05


def _pose(R, o):
    P = np.eye(4, dtype=np.float32)
    P[:3, :3], P[:3, 3] = R, o
    return P


def head_poses():
    eye = np.eye(3)
    rx = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])   # exact 90 degree turns
    ry = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0.0]])
    a = 0.7
    tilt = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ rx
    return np.stack([
        _pose(eye, (0, 0, 0)),                   # at the box centre
        _pose(ry, (0, 0, 0)),
        _pose(rx, (0.97, 0.97, -0.97)),          # near a corner
        _pose(tilt, (-0.4, 0.3, 0.2)),
        _pose(eye, (1.0, 0.3, -0.2)),            # on the x = +1 face: column 3 has d_x = 0, far = NaN
        _pose(eye, (-1.0, -0.1, 0.4)),           # on the x = -1 face: near = NaN
        _pose(rx, (0.2, -1.0, 0.1)),             # on a y face after a turn
        _pose(eye, (0.1, -0.2, 3.0)),            # outside, looking away (the camera looks down +z)
        _pose(eye, (0.0, 2.5, 0.0)),             # outside, looking past the box
    ]).astype(np.float32)


def _check_head(cuda, ro, rd, nears, fars, what):
    """nears / fars a head wrote against raymarching.near_far_from_aabb of the
    rays it wrote (the relation test_gather asserts), and against the oracle."""
    import raymarching
    aabb = torch.tensor(HEAD_AABB, device=cuda)
    n2, f2 = raymarching.near_far_from_aabb(ro, rd, aabb, HEAD_MIN_NEAR)
    n3, f3 = oracle.near_far_from_aabb(ro.cpu().numpy(), rd.cpu().numpy(), np.array(HEAD_AABB, np.float32), HEAD_MIN_NEAR)
    nears, fars = nears.cpu().numpy(), fars.cpu().numpy()
    assert_bits(nears, n2.cpu().numpy(), what + " nears vs k_near_far")
    assert_bits(fars, f2.cpu().numpy(), what + " fars vs k_near_far")
    assert_bits(nears, n3, what + " nears vs oracle")
    assert_bits(fars, f3, what + " fars vs oracle")
    return nears, fars


def _covers(nears, fars, rd):
    miss = fars == rc.FLT_MAX
    return dict(nan_near=int(np.isnan(nears).sum()), nan_far=int(np.isnan(fars).sum()), miss=int(miss.sum()),
                away=int((~miss & (fars < nears)).sum()), zeros=int((rd == 0).sum()),
                hit=int((~miss & (fars > nears)).sum()))


def test_frame_begin_near_far(cuda, parity_report):
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    poses = t(head_poses(), cuda)
    n, N = poses.shape[0], HW * HW
    intr, aabb = (ctypes.c_float * 4)(*INTR), (ctypes.c_float * 6)(*HEAD_AABB)
    tot = dict()
    for k in range(n):
        f = {name: torch.full((N, w) if w > 1 else (N,), -7.0, device=cuda)
             for name, w in (("rays_o", 3), ("rays_d", 3), ("nears", 1), ("fars", 1), ("noises", 1), ("rays_t", 1),
                             ("weights_sum", 1), ("depth", 1), ("image", 3))}
        alive = torch.full((N,), -7, dtype=torch.int32, device=cuda)
        state = torch.zeros(int(lib.ngp_render_state_bytes()), dtype=torch.uint8, device=cuda)
        nat.check(lib.ngp_frame_begin(P(poses), n, k, intr, HW, HW, aabb, HEAD_MIN_NEAR, P(f["rays_o"]), P(f["rays_d"]),
                                      P(f["nears"]), P(f["fars"]), P(f["noises"]), P(alive), P(f["rays_t"]),
                                      P(f["weights_sum"]), P(f["depth"]), P(f["image"]), P(state),
                                      nat.stream_of(poses)), "frame_begin")
        assert torch.equal(f["rays_o"], poses[k, :3, 3].expand(N, 3))
        nears, fars = _check_head(cuda, f["rays_o"], f["rays_d"], f["nears"], f["fars"], f"pose {k}")
        assert_bits(f["rays_t"].cpu().numpy(), nears, "rays_t")
        for key, v in _covers(nears, fars, f["rays_d"].cpu().numpy()).items():
            tot[key] = tot.get(key, 0) + v
    parity_report(f"{n} poses x {N} pixels: {tot}")
    assert tot["nan_near"] >= HW and tot["nan_far"] >= HW and tot["miss"] >= N and tot["away"] >= N
    assert tot["zeros"] >= 4 * HW and tot["hit"] >= 3 * N


def test_image_rays_near_far(cuda, parity_report):
    """The training draw's head, one pose at a time so every pose is drawn."""
    import _ngp_native as nat
    lib, P, n_rays = nat.lib(), nat.ptr, 256
    poses = t(head_poses(), cuda)
    intr, aabb = (ctypes.c_float * 4)(*INTR), (ctypes.c_float * 6)(*HEAD_AABB)
    pixels = torch.zeros(1, HW, HW, 4, dtype=torch.uint8, device=cuda)
    tot = dict()
    for k in range(poses.shape[0]):
        f = {name: torch.full((n_rays, w) if w > 1 else (n_rays,), -7.0, device=cuda)
             for name, w in (("rays_o", 3), ("rays_d", 3), ("rgba", 4), ("bg", 3), ("nears", 1), ("fars", 1),
                             ("noises", 1))}
        pix = torch.full((n_rays,), -1, dtype=torch.int32, device=cuda)
        index = torch.full((1,), -1, dtype=torch.int32, device=cuda)
        counter = torch.zeros(2, dtype=torch.int32, device=cuda)
        state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
        s = nat.stream_of(state)
        nat.check(lib.ngp_fused_state_init(P(state), 65536.0, s), "fused_state_init")
        src = nat.ImageSource()
        src.pixels, src.channels, src.dtype = P(pixels), 4, nat.DTYPE_U8
        src.pix, src.image_index = P(pix), P(index)
        pose = poses[k:k + 1].contiguous()
        nat.check(lib.ngp_image_rays(P(pose), 1, intr, HW, HW, n_rays, ctypes.byref(src), aabb, HEAD_MIN_NEAR, 11 + k,
                                     P(state), P(f["rays_o"]), P(f["rays_d"]), P(f["rgba"]), P(f["bg"]), P(f["nears"]),
                                     P(f["fars"]), P(f["noises"]), P(counter), None, s), "image_rays")
        assert pix.unique().numel() > HW * HW // 2
        nears, fars = _check_head(cuda, f["rays_o"], f["rays_d"], f["nears"], f["fars"], f"pose {k}")
        for key, v in _covers(nears, fars, f["rays_d"].cpu().numpy()).items():
            tot[key] = tot.get(key, 0) + v
    parity_report(f"{poses.shape[0]} poses x {n_rays} drawn rays: {tot}")
    assert tot["nan_near"] >= 1 and tot["nan_far"] >= 1 and tot["miss"] >= n_rays and tot["away"] >= n_rays
    assert tot["zeros"] >= HW and tot["hit"] >= 3 * n_rays
