"""GPU: the background model's backward at its own entry
(ngp_background_backward: k_bg_backward + k_bg_finish, csrc/background.hip)
against the float64 reference of tests/background_helpers.py, element by
element, on the cases of tests/background_cases.py: level 0 through global
atomics (lds0 off), a hashed level 0 inside the LDS copy, the second pass of
the block-strided loop, rays = nullptr, permuted rays lists and lists with
entries outside [0, N), N below a wave and around a workgroup; the order
independence of the integer sums, the finishing pass's fp16 overflow flag, and
the forward on the poles, the seam, rays from the centre and both other grids.

Tolerance per element (background_helpers.backward_tolerance):
    4 * 2^-11 * S_i + n_i * 2^-25 + fp16 spacing at |ref_i|
S_i the reference's expression with absolute values from gy on, n_i the scatter
terms on a table entry or the workgroups for dW: one missing or doubled ray on
an entry that fewer than about 100 rays touch exceeds it.

The reference's ReLU mask is certain on the case builder's float64 input rows.
The rows the forward kernel saves differ from those in a few fp16 ulps, so the
mask is checked again on x_save itself; a ray that has an uncertain unit there
is given out_ws = 1 (its gradient is then exactly zero in kernel and reference,
whatever the mask) and counted."""
import numpy as np
import pytest
import torch

import background_cases as bc
import background_helpers as bh

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in bc.CASES]


def _nat():
    import _ngp_native as nat
    return nat


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a copy: the shared case data is read-only)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


class Entry:
    """The two entries on one case's grid and weights, the parameters built
    directly (a 2-D GridEncoder for its offsets, the flat fp16 weights)."""

    def __init__(self, dev, name):
        from gridencoder import GridEncoder
        self.nat, self.dev, self.case, self.d = _nat(), dev, bc.BY_NAME[name], bc.case_data(name)
        d = self.d
        self.enc = GridEncoder(input_dim=2, num_levels=4, level_dim=2, base_resolution=d["base"],
                               log2_hashmap_size=self.case.log2T, desired_resolution=bc.DESIRED).to(dev)
        assert self.enc.offsets.tolist() == d["offsets"] and float(np.log2(self.enc.per_level_scale)) == d["S"]
        self.grid = (4, 2, d["S"], d["base"])
        self.table = _dev(d["table"], dev)
        self.weights = _dev(d["weights"], dev)
        self.values = self.table.numel()
        lib = self.nat.lib()
        self.state = torch.zeros(int(lib.ngp_fused_state_bytes()), dtype=torch.uint8, device=dev)
        self.nat.check(lib.ngp_fused_state_init(self.nat.ptr(self.state), 1.0, self.nat.stream_of(self.state)),
                       "fused_state_init")
        self.flag = lib.ngp_fused_inf_flag(self.nat.ptr(self.state), 0)
        self.scratch = torch.zeros(int(lib.ngp_background_scratch_bytes(self.values)), dtype=torch.uint8, device=dev)

    def forward(self, o, d, table=None):
        """-> bg [N, 3], x_save [N, 32] half, sph_save [N, 2]."""
        nat, P, N = self.nat, self.nat.ptr, o.shape[0]
        table = self.table if table is None else table
        bg = torch.full((N, 3), -1.0, device=self.dev)
        xs = torch.full((N, 32), 7.0, dtype=torch.float16, device=self.dev)
        sp = torch.full((N, 2), -7.0, device=self.dev)
        nat.check(nat.lib().ngp_background_forward(
            P(o), P(d), bc.RADIUS, N, P(table), nat.DTYPE_CODE[table.dtype], P(self.enc.offsets), *self.grid,
            P(self.weights), 32, 64, 2, P(bg), None, P(xs), P(sp), None, None, nat.stream_of(bg)),
            "background_forward")
        torch.cuda.synchronize()
        return bg, xs, sp

    def backward(self, rays, N, out_image, out_ws, gt, bg, xs, sp, scale=bc.SCALE, color_weight=1.0):
        """-> grad_table [entries, 2], grad_weights [3072] (numpy, float64 of
        the half values), the found-inf flag; the scratch must come back zero."""
        nat, P = self.nat, self.nat.ptr
        self.state.view(torch.float32)[0] = scale
        self.state.view(torch.int32)[5] = 0
        gtab = torch.full((self.values // 2, 2), 7.0, dtype=torch.float16, device=self.dev)  # (canaries: every value is written)
        gw = torch.full((3072,), 7.0, dtype=torch.float16, device=self.dev)
        nat.check(nat.lib().ngp_background_backward(
            P(rays), N, P(out_image), P(out_ws), P(gt), P(bg), P(xs), P(sp), P(self.enc.offsets), *self.grid,
            self.values, P(self.weights), 32, 64, 2, P(self.state), float(color_weight), bc.RADIUS, P(self.scratch),
            P(gtab), P(gw), self.flag, nat.stream_of(gtab)), "background_backward")
        torch.cuda.synchronize()
        assert not bool(self.scratch.any())
        return gtab, gw, int(self.state.view(torch.int32)[5])


def _inputs(entry, dev):
    """The case on the device: the forward's saved values, the composite's
    buffers and the rays list; rays with an uncertain unit in x_save get
    out_ws = 1. -> (dict of device tensors, the same as numpy, rays masked)."""
    d, N = entry.d, entry.d["N"]
    o, dd = _dev(d["o"], dev), _dev(d["d"], dev)
    bg, xs, sp = entry.forward(o, dd)
    out_ws = np.array(d["out_ws"])
    masked = np.flatnonzero(bh.uncertain_units(xs.cpu().numpy(), d["weights"]).any(1))
    assert masked.size <= max(1, N // 100) and masked.size < N, masked
    out_ws[masked] = 1.0
    t = dict(rays=None if d["rays"] is None else _dev(d["rays"], dev), out_image=_dev(d["out_image"], dev),
             out_ws=_dev(out_ws, dev), gt=_dev(d["gt"], dev), bg=bg, xs=xs, sp=sp)
    host = {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}
    return t, host, int(masked.size)


def _reference(entry, host, order, scale=bc.SCALE, color_weight=None, faithful=True):
    d = entry.d
    cw = entry.case.color_weight if color_weight is None else color_weight
    return bh.background_backward64(host["xs"], host["sp"], host["bg"], host["out_image"], host["out_ws"], host["gt"],
                                    d["weights"], scale, cw, d["N"], d["offsets"], d["base"], d["S"], order=order,
                                    faithful=faithful)


def _compare(gtab, gw, ref):
    """Every element within its tolerance; entries no ray touches and rows
    3..15 of W1 exactly zero. -> the worst error / tolerance of each tensor."""
    r_table, r_w0, r_w1, b = ref
    got_t = gtab.cpu().numpy().astype(np.float64)
    got_w = gw.cpu().numpy().astype(np.float64)
    assert np.isfinite(got_t).all() and np.isfinite(got_w).all()
    assert not got_w[2048 + 3 * 64:].any()
    untouched = b["n_table"] == 0
    assert not got_t[untouched].any()
    assert not _bits(gtab).cpu().numpy()[untouched].any()  # (+0, not -0)
    ratios = {}
    for what, got, want, S, n in (("table", got_t, r_table, b["S_table"], b["n_table"][:, None]),
                                  ("dW0", got_w[:2048].reshape(64, 32), r_w0, b["S_w0"], b["n_w"]),
                                  ("dW1", got_w[2048:2048 + 192].reshape(3, 64), r_w1, b["S_w1"], b["n_w"])):
        ratio = np.abs(got - want) / bh.backward_tolerance(want, S, n)
        ratios[what] = float(ratio.max())
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{what}: worst error / tolerance {ratios[what]:.3f} at {at}: got {got[at]:.6e} want {want[at]:.6e} "
              f"S {S[at]:.3e}; max |ref| {np.abs(want).max():.3e}, nonzero {int((want != 0).sum())}")
    for what, r in ratios.items():
        assert r <= 1.0, (what, r)
    return ratios


@pytest.fixture(scope="module")
def entries(cuda):
    cache = {}

    def get(name):
        if name not in cache:
            e = Entry(cuda, name)
            cache[name] = (e,) + _inputs(e, cuda)
        return cache[name]
    return get


# ---- 1. against float64 ----------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_backward_matches_float64(cuda, entries, parity_report, name):
    """grad_table, dW0 and rows 0..2 of dW1 against background_backward64(
    faithful=True) on what the kernel read, element-wise within the tolerance;
    untouched entries and rows 3..15 of W1 exactly 0, the flag clear, the
    scratch left zero. second_pass (out_ws = 1 exactly below 16384: only the
    loop's second pass contributes) is held to the reference of its 65 live
    rays, second_pass_all to that of all 16449."""
    entry, t, host, masked = entries(name)
    d, N = entry.d, entry.d["N"]
    gtab, gw, flag = entry.backward(t["rays"], N, t["out_image"], t["out_ws"], t["gt"], t["bg"], t["xs"], t["sp"],
                                    color_weight=entry.case.color_weight)
    assert flag == 0
    order = bc.order_of(d)
    if entry.case.live == "tail":
        assert order is None and (host["out_ws"][:bc.ONE_PASS] == 1).all()
        order = np.arange(bc.ONE_PASS, N)
    ref = _reference(entry, host, order)
    assert np.abs(ref[0]).max() > 0 and (ref[3]["n_table"] > 0).sum() >= 4
    ratios = _compare(gtab, gw, ref)
    parity_report(f"{name}: N {N}, {int((ref[3]['n_table'] > 0).sum())} entries touched, {d['redrawn']} rays redrawn, "
                  f"{masked} masked; worst error / tolerance table {ratios['table']:.3f} dW0 {ratios['dW0']:.3f} "
                  f"dW1 {ratios['dW1']:.3f}")


# ---- 2. order independence -------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "second_pass_all"])
def test_order_independence(cuda, entries, name):
    """The same inputs under two permutations of the rays list and under the
    identity (rays = nullptr): grad_table bit-identical (each contribution is
    quantised on its own and integer sums commute), whichever wave, workgroup
    or loop pass takes a ray. Two runs with the same list: both gradients
    bit-identical. (dW is not compared across lists: its in-wave fp32 order
    changes with the assignment of rays to waves.)"""
    entry, t, host, _ = entries(name)
    N = entry.d["N"]
    rng = np.random.default_rng(5)
    lists = []
    for _ in range(2):
        rays = rng.integers(0, 1 << 20, (N, 3)).astype(np.int32)
        rays[:, 0] = rng.permutation(N)
        lists.append(_dev(rays, cuda))
    assert not torch.equal(lists[0][:, 0], lists[1][:, 0])
    run = lambda rays: entry.backward(rays, N, t["out_image"], t["out_ws"], t["gt"], t["bg"], t["xs"], t["sp"],  # noqa: E731
                                      color_weight=entry.case.color_weight)
    a, a2, b, c = run(lists[0]), run(lists[0]), run(lists[1]), run(None)
    assert a[2] == a2[2] == b[2] == c[2] == 0
    assert float(a[0].float().abs().max()) > 0 and float(a[1].float().abs().max()) > 0
    assert torch.equal(_bits(a[0]), _bits(a2[0])) and torch.equal(_bits(a[1]), _bits(a2[1]))
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[0]), _bits(c[0]))


# ---- 3. fp16 overflow in the finishing pass ------------------------------------------------
def test_finish_overflow_flag(cuda, entries, parity_report):
    """1024 copies of one ray. With the scale at which the float64 sum on the
    hottest level-0 entry is 2.2 x 65504 every contribution is finite and below
    1e3 (far inside add_fixed's guard), so only k_bg_finish can raise the flag,
    and it must; with every sum at most 65504 / 2 the flag stays clear and the
    values meet the tolerance."""
    entry, _, _, _ = entries("default")
    d, N = entry.d, 1024
    o, dd = (_dev(np.repeat(d[k][3:4], N, 0), cuda) for k in ("o", "d"))
    bg, xs, sp = entry.forward(o, dd)
    assert not bh.uncertain_units(xs[:1].cpu().numpy(), d["weights"]).any()
    out_image = torch.full((N, 3), 0.9, device=cuda)
    gt = torch.tensor([0.1, 0.3, 0.2, 1.0], device=cuda).repeat(N, 1)
    out_ws = torch.zeros(N, device=cuda)
    host = {k: v.cpu().numpy() for k, v in dict(xs=xs, sp=sp, bg=bg, out_image=out_image, gt=gt, out_ws=out_ws).items()}

    def reference(scale, faithful):
        return bh.background_backward64(host["xs"], host["sp"], host["bg"], host["out_image"], host["out_ws"],
                                        host["gt"], d["weights"], scale, 1.0, N, d["offsets"], d["base"], d["S"],
                                        faithful=faithful)
    unit = reference(1.0, False)
    lvl0 = np.abs(unit[0][:d["offsets"][1]])
    hot = np.unravel_index(int(lvl0.argmax()), lvl0.shape)
    hi = 2.2 * 65504 / lvl0[hot]
    lo = 0.49 * 65504 / max(np.abs(u).max() for u in unit)
    # every scatter term of the identical rays is 1 / 1024 of its entry's sum (fewer terms on an entry only lower it)
    assert hi * np.abs(unit[0]).max() / N < 1e3 and hi * lvl0[hot] >= 2 * 65504 and lo * lvl0[hot] <= 65504 / 2
    top = reference(hi, True)
    assert all(np.isfinite(v).all() for v in top[:3]) and np.abs(top[0][hot]) >= 2 * 65504  # gy, delta, gi inside fp16
    gtab, gw, flag = entry.backward(None, N, out_image, out_ws, gt, bg, xs, sp, scale=hi)
    assert flag & 1 and bool(torch.isinf(gtab[hot[0], hot[1]]))
    gtab, gw, flag = entry.backward(None, N, out_image, out_ws, gt, bg, xs, sp, scale=lo)
    assert flag == 0
    ratios = _compare(gtab, gw, reference(lo, True))
    parity_report(f"scale {hi:.4g}: flag raised, level-0 sum {hi * lvl0[hot]:.4g}; scale {lo:.4g}: clear, worst error / "
                  f"tolerance table {ratios['table']:.3f} dW0 {ratios['dW0']:.3f} dW1 {ratios['dW1']:.3f}")


# ---- 4. the forward on the edge rays and the other grids ----------------------------------------
@pytest.mark.parametrize("name", bc.FORWARD_CASES)
def test_forward_edges(cuda, entries, parity_report, name):
    """The poles, the seam (phi = +-pi: x1 = 1 or 0, pg + 1 == res), rays from
    the centre, and the grids with level 0 past the LDS limit and hashed: the
    kernel's error against background64 is at most twice the autograd ops' on
    the same rays (test_forward_matches_float64_and_autograd's rule; 2 * 2^-11
    where both are zero), also ray by ray with that floor; sph_save is
    (sph_from_ray + 1) / 2 bit for bit; the fp16 and fp32 tables give the same
    bits."""
    import raymarching
    from nerf.network_ff import BackgroundMLP
    from shencoder import SHEncoder
    entry, t, host, _ = entries(name)
    d = entry.d
    o, dd = _dev(d["o"], cuda), _dev(d["d"], cuda)
    bg, xs, sp = t["bg"], t["xs"], t["sp"]
    assert torch.isfinite(bg).all() and float(bg.min()) >= 0 and float(bg.max()) <= 1
    bg32, xs32, sp32 = entry.forward(o, dd, table=entry.table.float())
    assert torch.equal(_bits(bg), _bits(bg32)) and torch.equal(_bits(xs), _bits(xs32)) and torch.equal(sp, sp32)
    sph = raymarching.sph_from_ray(o, dd, bc.RADIUS)
    assert torch.equal(_bits(sp), _bits((sph + 1) / 2))

    want = bh.background64(d["o"], d["d"], bc.RADIUS, d["table"], d["weights"], d["offsets"], d["base"], d["S"])
    net, sh = BackgroundMLP().to(cuda), SHEncoder(input_dim=3, degree=4).to(cuda)
    with torch.no_grad():
        net.weights.copy_(entry.weights.float())
        entry.enc.embeddings.copy_(entry.table.float())
        with torch.autocast("cuda", dtype=torch.float16):
            feat = torch.cat([sh(dd), entry.enc(sph), torch.zeros(d["N"], 8, dtype=torch.float16, device=cuda)], -1)
            auto = torch.sigmoid(net(feat))
    assert auto.dtype == torch.float16 and auto.shape == (d["N"], 3)
    err_auto = np.abs(auto.double().cpu().numpy() - want).max(1)
    err = np.abs(bg.double().cpu().numpy() - want).max(1)
    floor = 2 * 2.0 ** -11
    if name == "named_rays":
        names, _, _ = bc.named_rays()
        for k, what in enumerate(names):
            print(f"{what:26s} sph01 {host['sp'][k, 0]:.9g} {host['sp'][k, 1]:.9g}  err kernel {err[k]:.3e} "
                  f"autograd ops {err_auto[k]:.3e}")
    print(f"{name}: max |err| against float64: kernel {err.max():.3e}, autograd ops {err_auto.max():.3e}")
    parity_report(f"{name}: forward max |err| against float64: kernel {err.max():.3e}, autograd ops "
                  f"{err_auto.max():.3e}")
    assert err.max() <= (2 * err_auto.max() if err_auto.max() > 0 else floor)
    assert (err <= np.maximum(2 * err_auto, floor)).all(), np.flatnonzero(err > np.maximum(2 * err_auto, floor))
