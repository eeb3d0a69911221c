"""GPU: the fused optimizer and loss scaler (adam_sweep / adam_sweep_pipe,
k_nonfinite, step_end_block, ngp_adam_step) against the float64 reference and
the scaler machine of tests/optimizer_cases.py, through direct C-ABI calls on
small ragged tensor lists inside canaried buffers, over a schedule that grows,
backs off and skips.

Tolerance of p / m / v: against adam_reference_f64, at
most 4 x the float32 restatement's own error of the same case and tensor kind
(floor: 1 ulp32 of the reference value), per value and in relative norm. The
share of values bit-identical to the restatement is reported, not asserted.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import optimizer_cases as oc

pytestmark = pytest.mark.gpu

OFF, SCAN, PRECHECKED = 0, 1, 2   # NGP_SCALER_OFF / _SCAN / _PRECHECKED
SHADOW_ALL = 2                    # NGP_ADAM_SHADOW_ALL (zero_grads bit 1)
# StepState words (csrc/ngp_step.h)
W_SCALE, W_LOSS_SUM, W_LAST_LOSS, W_TRACKER, W_INF, W_ADAM, W_EPOCH, W_ITER, W_PENDING = 0, 1, 2, 4, 5, 6, 7, 8, 12


def _nat():
    import _ngp_native as nat
    return nat


def _bits(a):
    a = np.asarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


class State:
    """A device StepState."""

    def __init__(self, cuda, scale=65536.0, **words):
        nat = _nat()
        assert nat.lib().ngp_fused_state_bytes() == 64
        self.buf = torch.zeros(16, dtype=torch.int32, device=cuda)
        nat.check(nat.lib().ngp_fused_state_init(self.buf.data_ptr(), float(scale), nat.stream_of(self.buf)), "init")
        # the found-inf word the backward's kernels (and these tests) write
        flag = nat.lib().ngp_fused_inf_flag(self.buf.data_ptr(), 0)
        assert flag == self.buf.data_ptr() + 4 * W_INF
        self.set(**words)

    def set(self, **words):
        for k, v in words.items():
            if k in ("scale", "loss_sum", "last_loss"):
                self.buf.view(torch.float32)[{"scale": 0, "loss_sum": 1, "last_loss": 2}[k]] = \
                    torch.tensor(np.float32(v).item(), dtype=torch.float32)
            else:
                self.buf[{"tracker": W_TRACKER, "found_inf": W_INF, "adam_step": W_ADAM, "epoch": W_EPOCH,
                          "iter": W_ITER, "end_pending": W_PENDING}[k]] = int(v)

    def read(self):
        torch.cuda.synchronize()
        i = self.buf.cpu().numpy()
        f = i.view(np.float32)
        return dict(scale=float(f[W_SCALE]), loss_sum=float(f[W_LOSS_SUM]), last_loss=float(f[W_LAST_LOSS]),
                    tracker=int(i[W_TRACKER]), found_inf=int(i[W_INF]), adam_step=int(i[W_ADAM]),
                    epoch=int(i[W_EPOCH]), iter=int(i[W_ITER]), end_pending=int(i[W_PENDING]))

    def machine_words(self):
        r = self.read()
        return (r["scale"], r["tracker"], r["adam_step"], r["epoch"], r["iter"])


class Dev:
    """A case's buffers on the device and the optimizer entries on them."""

    def __init__(self, case, cuda):
        self.case, self.cuda = case, cuda
        self.t = {}
        for kind in "pmvgh":
            self.upload(kind)
        self.counter = torch.zeros(2, dtype=torch.int32, device=cuda)

    def upload(self, kind, host=None):
        host = self.case.buf[kind] if host is None else host
        src = torch.from_numpy(host.view(np.int16) if kind in "gh" else host.view(np.float32))
        if kind in self.t:
            self.t[kind].copy_(src)
        else:
            self.t[kind] = src.to(self.cuda)
            assert self.t[kind].data_ptr() % 16 == 0

    def download(self):
        torch.cuda.synchronize()
        return {kind: _bits(t.cpu().numpy()) for kind, t in self.t.items()}

    def host_bits(self):
        return {kind: _bits(self.case.buf[kind]).copy() for kind in "pmvgh"}

    def arrays(self, n=None, shadows=True, shift=None):
        c = self.case
        n = c.n() if n is None else n
        vp = ctypes.c_void_p * n

        def ptrs(kind):
            size = 2 if kind in "gh" else 4
            out = [self.t[kind].data_ptr() + size * c.off[kind][k % c.n()] for k in range(n)]
            if shift and kind == shift[0]:
                out[0] += shift[1]
            if kind == "h":
                out = [q if shadows and c.has_shadow(k % c.n()) else None for k, q in enumerate(out)]
            return vp(*out)
        sizes = (ctypes.c_uint64 * n)(*[c.sizes[k % c.n()] for k in range(n)])
        return (n, ptrs("p"), ptrs("g"), ptrs("m"), ptrs("v"), ptrs("h"), sizes)

    def launch(self, st, entry="step", mode=SCAN, zero_grads=1, grad_mult=1.0, iters=30000, growth_interval=2000,
               n_rays=0, loss_ray=None, step_counter=None, arrays=None):
        nat = _nat()
        lib, P = nat.lib(), nat.ptr
        args = (arrays or self.arrays()) + (oc.LR, oc.B1, oc.B2, oc.EPS, iters, zero_grads, grad_mult)
        s = nat.stream_of(self.counter)
        if entry == "update":
            return lib.ngp_fused_optimizer_update(*args, mode, st.buf.data_ptr(), s)
        return lib.ngp_fused_optimizer_step(*args, 2.0, 0.5, growth_interval, mode, n_rays, P(self.counter),
                                            P(step_counter), P(loss_ray), st.buf.data_ptr(), s)

    def run(self, st, **kw):
        _nat().check(self.launch(st, **kw), "fused optimizer")


def _expand_idle(case):
    return [np.repeat(g, 4)[:n] for g, n in zip(case.groups(), case.sizes)]


def check_buffers(case, before, after, *, ref_pairs=None, skipped=False, zero_grads=1, report=None, label=""):
    """What one update may and must have done to the case's buffers.
    before / after: {kind: bits}; ref_pairs: per tensor (reference pmv float64,
    restated pmv float32) of an applied update, None: only the bit checks."""
    shadow_all = bool(zero_grads & SHADOW_ALL)
    for kind in "pmvgh":  # nothing outside the tensors: canaries before, between and behind them
        can = case.canary[kind]
        assert np.array_equal(after[kind][can], before[kind][can]), (label, kind, "canary touched",
                                                                    np.flatnonzero(after[kind][can] != before[kind][can])[:8])
    if case.padding is not None:  # the flat gradient's alignment padding is neither read nor written
        assert np.array_equal(after["g"][case.padding], before["g"][case.padding]), (label, "padding written")
    idle = _expand_idle(case)
    seams = oc.seam_masks(case.sizes)
    for k in range(case.n()):
        a = {kind: case.view(kind, k, after[kind]) for kind in "pmvgh"}
        b = {kind: case.view(kind, k, before[kind]) for kind in "pmvgh"}
        if zero_grads & 1:
            assert not a["g"].any(), (label, k, "gradient bits left", np.flatnonzero(a["g"])[:8])
        else:
            assert np.array_equal(a["g"], b["g"]), (label, k, "gradient changed")
        keep = np.ones(case.sizes[k], bool) if skipped else idle[k]
        for kind in "pmv":
            assert np.array_equal(a[kind][keep], b[kind][keep]), (label, k, kind, "idle or skipped values changed")
        if not skipped:
            moved = ~idle[k]
            if moved.any():
                assert not np.array_equal(a["p"][moved], b["p"][moved]), (label, k, "nothing moved")
        if not case.has_shadow(k):
            continue
        want = b["h"].copy()
        half_p = _bits(a["p"].view(np.float32).astype(np.float16))
        if shadow_all:
            want = half_p
        elif not skipped:
            # whole chunks write the shadow of the groups that moved; the per-element
            # seam loop writes every value's (deliberate divergences)
            wr = seams[k] | ~idle[k]
            want[wr] = half_p[wr]
        assert np.array_equal(a["h"], want), (label, k, "shadow", np.flatnonzero(a["h"] != want)[:8])
    if ref_pairs is None or skipped:
        return
    restated = oc.figures_over_tensors(ref_pairs)
    got_pairs = [(ref, tuple(case.view(kind, k, after[kind]).view(np.float32) for kind in "pmv"))
                 for k, (ref, _) in enumerate(ref_pairs)]
    same = []
    for i, kind in enumerate("pmv"):
        ref = np.concatenate([r[i] for r, _ in got_pairs])
        got = np.concatenate([g[i] for _, g in got_pairs])
        res = np.concatenate([np.asarray(r[i], np.float32) for _, r in ref_pairs])
        ok, fig, allowed = oc.within_margin(got, ref, restated[kind])
        print(f"[{label}] {kind}: device max {fig[0]:.2f} ulp32 rel-norm {fig[1]:.2e}; restatement "
              f"{restated[kind][0]:.2f} ulp32 {restated[kind][1]:.2e}; allowed {allowed[0]:.2f} ulp32 {allowed[1]:.2e}")
        assert ok, (label, kind, fig, allowed)
        same.append(float((_bits(got) == _bits(res)).mean()))
    if report:
        report(f"{label}: bit-identical to the float32 restatement p {same[0]:.4f} m {same[1]:.4f} v {same[2]:.4f}")


@functools.lru_cache(maxsize=None)
def _case(name, packed=False):
    return oc.make_case(name, packed=packed)


@functools.lru_cache(maxsize=None)
def _one_update(name, grad_mult=1.0):
    return oc.one_update(_case(name), grad_mult=grad_mult)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    for f in (_case, _one_update, _default_schedule):
        f.cache_clear()


# ---- 1, 2: one update on each ragged list ----------------------------------------------------------------
@pytest.mark.parametrize("zero_grads", [1, 1 | SHADOW_ALL])
@pytest.mark.parametrize("name", ["R8", "R4", "R1", "EPS"])
def test_one_update_of_each_ragged_list(cuda, parity_report, name, zero_grads):
    """ngp_fused_optimizer_step (NGP_SCALER_SCAN) once on each list: p / m / v
    within the margin, idle groups untouched, every gradient bit cleared,
    shadows (half(p) where the group moved; every value with
    NGP_ADAM_SHADOW_ALL; null shadows skipped), every canary intact."""
    case = _case(name)
    dev = Dev(case, cuda)
    st = State(cuda, case.scale)
    before = dev.host_bits()
    dev.run(st, zero_grads=zero_grads)
    after = dev.download()
    mach = oc.ScalerMachine(case.scale)
    assert not mach.update(0)
    assert st.machine_words() == mach.state() and st.read()["found_inf"] == 0
    check_buffers(case, before, after, ref_pairs=_one_update(name), zero_grads=zero_grads,
                  report=parity_report, label=f"{name} zero_grads {zero_grads}")


@pytest.mark.parametrize("name", ["R8", "R4"])
def test_shadow_all_on_a_skipped_update(cuda, name):
    """NGP_ADAM_SHADOW_ALL writes half(p) into every shadow value on a skipped
    update too, in whole chunks and in seam chunks; without it a skipped update
    leaves the shadows alone."""
    case = _case(name)
    for zg in (1 | SHADOW_ALL, 1):
        dev = Dev(case, cuda)
        st = State(cuda, case.scale)
        k, off = oc.inf_candidates(case)[-1]
        host = case.buf["g"].copy()
        case.view("g", k, host)[off] = oc.NONFINITE16["+inf"]
        dev.upload("g", host)
        before = dev.host_bits()
        before["g"] = host
        dev.run(st, zero_grads=zg)
        assert st.machine_words() == (case.scale / 2, 0, 0, 1, 1)
        check_buffers(case, before, dev.download(), skipped=True, zero_grads=zg, label=f"{name} skipped zg {zg}")


# ---- 3: the schedule ---------------------------------------------------------------------------------------
def test_schedule_through_fused_optimizer_step(cuda, parity_report):
    """14 updates of R4 with growth_interval 3 and iters 8, an inf in updates
    {2, 6, 7, 11} (another place each time): after every update the state
    words equal ScalerMachine exactly; a skipped update keeps p / m / v and
    the shadows and clears the gradient, the inf too; the end state is within
    the margin of the float64 reference carried through the same schedule with
    the machine's scale and its own step and epoch counts."""
    s, case = oc.SCHEDULE, _case("R4")
    dev, st = Dev(case, cuda), State(cuda, s["init_scale"])
    mach = oc.ScalerMachine(s["init_scale"], growth_interval=s["growth_interval"])
    states, pairs = oc.run_schedule(case)
    for it in range(s["K"]):
        inf = it in s["inf_updates"]
        grads = oc.fresh_grads(case, it, float(mach.scale))
        host = case.buf["g"].copy()
        for k in range(case.n()):
            case.view("g", k, host)[:] = grads[k]
        if inf:
            k, off = oc.schedule_inf_place(case, it)
            case.view("g", k, host)[off] = list(oc.NONFINITE16.values())[it % 3]
        dev.upload("g", host)
        before = dev.download()
        dev.run(st, iters=s["iters"], growth_interval=s["growth_interval"])
        assert mach.update(0 if not inf else 1) == inf
        assert st.machine_words() == mach.state() == states[it], (it, st.machine_words(), mach.state())
        assert st.read()["found_inf"] == 0
        after = dev.download()
        if inf:
            check_buffers(case, before, after, skipped=True, label=f"schedule update {it}")
        else:
            assert not any(case.view("g", k, after["g"]).any() for k in range(case.n()))
    assert tuple(int(x) for x in mach.state()[:4]) == oc.TRAJECTORY[-1]
    restated = oc.figures_over_tensors(pairs)
    same = []
    for i, kind in enumerate("pmv"):
        ref = np.concatenate([r[i] for r, _ in pairs])
        res = np.concatenate([np.asarray(q[i], np.float32) for _, q in pairs])
        got = np.concatenate([case.view(kind, k, after[kind]).view(np.float32) for k in range(case.n())])
        ok, fig, allowed = oc.within_margin(got, ref, restated[kind])
        print(f"[schedule] {kind}: device max {fig[0]:.2f} ulp32 rel-norm {fig[1]:.2e}; restatement "
              f"{restated[kind][0]:.2f} ulp32 {restated[kind][1]:.2e}")
        assert ok, (kind, fig, allowed)
        same.append(float((_bits(got) == _bits(res)).mean()))
    parity_report(f"R4 schedule, 10 applied updates: bit-identical to the float32 restatement "
                  f"p {same[0]:.4f} m {same[1]:.4f} v {same[2]:.4f}")
    host = dev.host_bits()
    for kind in "pmvgh":
        assert np.array_equal(after[kind][case.canary[kind]], host[kind][case.canary[kind]]), kind
    # (every gradient touched every group, so there is no idle group left: every shadow value is half(p))
    for k in range(case.n()):
        if case.has_shadow(k):
            p = case.view("p", k, after["p"]).view(np.float32)
            assert np.array_equal(case.view("h", k, after["h"]), _bits(p.astype(np.float16))), k


# ---- 4: k_nonfinite by position ----------------------------------------------------------------------------
def _skips(dev, st, case, host, scale=65536.0):
    """One NGP_SCALER_SCAN update of `host`'s gradients -> whether it skipped
    (and then: backed off once, tracker reset, no Adam step, gradient cleared)."""
    dev.upload("g", host)
    st.set(scale=scale, tracker=1, adam_step=0, epoch=0, iter=0)
    dev.run(st)
    w = st.machine_words()
    assert st.read()["found_inf"] == 0
    if w[2] == 1:
        assert w == (scale, 2, 1, 1, 1), w
        return False
    assert w == (scale / 2, 0, 0, 1, 1), w
    return True


@pytest.mark.parametrize("name", ["R8", "R4"])
def test_nonfinite_found_at_every_edge(cuda, name):
    """+inf, -inf and NaN, one at a time, at the first and last element of
    every tensor (the last of a size % 8 != 0 tensor is read by the scalar
    tail) and inside the gradient whose pointer is only 8-byte aligned: each
    skips and backs off once, leaves p / m / v alone and is cleared; the
    clean gradient does not skip (no value behind a tensor's end is read:
    the canaries there are NaN)."""
    case = _case(name)
    dev, st = Dev(case, cuda), State(cuda)
    places = oc.inf_candidates(case)
    assert {case.nonfinite_path(*c) for c in places} == {"scalar", "vector"}
    zero = case.buf["g"].copy()
    for k in range(case.n()):
        case.view("g", k, zero)[:] = 0  # (a clean update of +0 gradients and the case's moments)
    before = dev.host_bits()
    for k, off in places:
        for what, bits in oc.NONFINITE16.items():
            host = zero.copy()
            case.view("g", k, host)[off] = bits
            assert _skips(dev, st, case, host), (name, k, off, what, case.nonfinite_path(k, off))
    after = dev.download()
    before["g"] = zero
    check_buffers(case, before, after, skipped=True, label=f"{name} nonfinite")
    assert not _skips(dev, st, case, case.buf["g"].copy()), "a clean gradient skipped"


def test_nonfinite_in_the_padding_between_tensors_does_not_skip(cuda):
    """The R8 gradients packed in one flat buffer the way make_list lays the
    tensors out (each start 8-aligned): a non-finite value in the alignment
    padding between two tensors is not part of any gradient. The kernels never
    read padding, so it must neither skip the update nor be cleared."""
    case = _case("R8", True)
    dev, st = Dev(case, cuda), State(cuda)
    assert case.padding.sum() == sum((-n) % 8 for n in case.sizes)
    host = case.buf["g"].copy()
    host[case.padding] = np.resize(np.array(list(oc.NONFINITE16.values()), np.uint16), int(case.padding.sum()))
    before = dev.host_bits()
    before["g"] = host
    assert not _skips(dev, st, case, host)
    check_buffers(case, before, dev.download(), ref_pairs=_one_update("R8"), label="R8 packed")
    # ... and one in a real element of the same buffer does
    host2 = host.copy()
    case.view("g", 3, host2)[4] = oc.NONFINITE16["nan"]
    assert _skips(dev, st, case, host2)


@pytest.fixture(scope="module")
def rbig(cuda):
    """RBIG on the host and the device (240 MB each), for this module only."""
    case = oc.make_case("RBIG")
    yield case, Dev(case, cuda)


def test_nonfinite_on_the_second_trip_of_the_grid_stride_loop(cuda, rbig):
    """RBIG is longer than k_nonfinite's grid (8192 x 256 x 8 values): its very
    last element, read on a thread's second trip, in the scalar tail."""
    case, dev = rbig
    st = State(cuda)
    assert case.flat_index(0, case.sizes[0] - 1) >= oc.NONFINITE_CAP
    host = np.zeros_like(case.buf["g"])
    host[case.canary["g"]] = case.buf["g"][case.canary["g"]]
    for what, bits in oc.NONFINITE16.items():
        case.view("g", 0, host)[-1] = bits
        assert _skips(dev, st, case, host), what
    case.view("g", 0, host)[-1] = 0
    assert not _skips(dev, st, case, host)


# ---- 5: the flag written by the caller ----------------------------------------------------------------------
def test_prechecked_flag_values(cuda):
    """NGP_SCALER_PRECHECKED with the found-inf word written before the launch:
    1 behaves as an inf; 2 (the gradient exchange overflowed) skips Adam, leaves
    scale and growth tracker as they were, does not bump adam_step, bumps epoch
    and iter and clears the flag, and with the tracker at growth_interval - 1
    the following clean update grows; 3 backs off."""
    case = _case("R4")
    for flags in ([0, 0, 2, 0], [1, 0], [0, 3, 0, 0, 2, 2, 0]):
        dev, st = Dev(case, cuda), State(cuda, 1024.0)
        mach = oc.ScalerMachine(1024.0, growth_interval=3)
        for it, flag in enumerate(flags):
            dev.upload("g")
            st.set(found_inf=flag)
            before = dev.download()
            dev.run(st, mode=PRECHECKED, growth_interval=3)
            was = mach.state()
            assert mach.update(flag) == (flag != 0)
            assert st.machine_words() == mach.state(), (flags, it)
            assert st.read()["found_inf"] == 0
            if flag:
                check_buffers(case, before, dev.download(), skipped=True, label=f"flag {flag}")
            if flag == 2:
                assert mach.state()[:3] == was[:3] and mach.state()[3:] == (was[3] + 1, was[4] + 1)
        if flags[:3] == [0, 0, 2]:
            assert mach.state() == (2048.0, 0, 3, 4, 4)  # tracker 2 survived the exchange overflow, then grew


# ---- 6: the scaler off --------------------------------------------------------------------------------------
def test_scaler_off_freezes_scale_and_tracker(cuda):
    """NGP_SCALER_OFF: scale and tracker stay over a clean and an inf-flagged
    update (growth_interval 1 would grow at once), the flagged one still
    skips, the step counts move as with the scaler on, and the gradients are
    still divided by the frozen scale."""
    case = _case("R4")
    dev, st = Dev(case, cuda), State(cuda, case.scale)
    before = dev.host_bits()
    dev.run(st, mode=OFF, growth_interval=1)
    assert st.machine_words() == (case.scale, 0, 1, 1, 1)
    after = dev.download()
    check_buffers(case, before, after, ref_pairs=_one_update("R4"), label="R4 scaler off")
    dev.upload("g")
    st.set(found_inf=1)
    before = dev.download()
    dev.run(st, mode=OFF, growth_interval=1)
    assert st.machine_words() == (case.scale, 0, 1, 2, 2) and st.read()["found_inf"] == 0
    check_buffers(case, before, dev.download(), skipped=True, label="R4 scaler off, flagged")
    mach = oc.ScalerMachine(case.scale, growth_interval=1, enabled=False)
    mach.update(0), mach.update(1)
    assert st.machine_words() == mach.state()


# ---- 7: grad_mult -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_mult", [1 / 3, 1 / 8])
@pytest.mark.parametrize("name", ["R8", "R4"])
def test_grad_mult(cuda, parity_report, name, grad_mult):
    case = _case(name)
    dev, st = Dev(case, cuda), State(cuda, case.scale)
    before = dev.host_bits()
    dev.run(st, grad_mult=grad_mult)
    check_buffers(case, before, dev.download(), ref_pairs=_one_update(name, grad_mult), report=parity_report,
                  label=f"{name} grad_mult {grad_mult:.4f}")


# ---- 8: 1 / scale not finite ----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step", "update"])
@pytest.mark.parametrize("scale", [0.0, 1e-39])
def test_unscale_overflow_skips_and_backs_off(cuda, scale, entry):
    """scale 0 and a float32 subnormal scale (1 / scale overflows float32):
    the finite fp16 gradients cannot show it, the sweep itself flags the inf:
    skip, back off, p / m / v untouched."""
    case = _case("R4")
    dev, st = Dev(case, cuda), State(cuda, scale, tracker=2)
    mach = oc.ScalerMachine(scale, growth_interval=3)
    mach.tracker = 2
    assert mach.unscale_overflows() and mach.update(0)
    before = dev.host_bits()
    dev.run(st, entry=entry, growth_interval=3)
    check_buffers(case, before, dev.download(), skipped=True, label=f"scale {scale}")
    if entry == "update":  # the bookkeeping is deferred: the sweep left the flag for it
        r = st.read()
        assert (r["found_inf"], r["end_pending"], r["adam_step"], r["epoch"], r["tracker"]) == (1, 1, 0, 0, 2)
        assert r["scale"] == float(np.float32(scale))
    else:
        assert st.machine_words() == mach.state(), (st.machine_words(), mach.state())
        assert st.read()["found_inf"] == 0


# ---- 9: loss and ring ------------------------------------------------------------------------------------------
def test_loss_mean_and_step_counter_ring(cuda):
    """step_end_block's loss sum (16 clamped loads per thread, then a 256-wide
    tree) around n_rays = 256 and 4096: last_loss within 3e-6 relative of
    sum64 / n_rays (at most 32 serial adds per thread + 8 tree levels on
    positive partial sums, 2^-24 relative each, + the multiply by the float32
    1 / n: 41 x 6e-8 = 2.5e-6), exactly 0 at n_rays = 0, loss_sum 0 afterwards.
    step_counter[iter % 16] takes each update's counter pair: 18 updates wrap it."""
    case = _case("R1")
    dev, st = Dev(case, cuda), State(cuda)
    rng = np.random.default_rng(11)
    ring = torch.full((32,), -1, dtype=torch.int32, device=cuda)
    sizes = [1, 255, 256, 257, 4095, 4096, 4097, 8191, 0]
    pairs = []
    for it in range(18):
        n = sizes[it % len(sizes)]
        host = (rng.random(n + 3) * 0.1 + 1e-3).astype(np.float32)
        host[n:] = 1e6  # behind the rays: never summed (the clamped loads re-read the last ray instead)
        loss = torch.from_numpy(host).to(cuda)
        pairs.append((10 * it + 1, 10 * it + 2))
        dev.counter.copy_(torch.tensor(pairs[-1], dtype=torch.int32))
        dev.upload("g")
        dev.run(st, n_rays=n, loss_ray=loss, step_counter=ring)
        r = st.read()
        assert r["iter"] == it + 1 and r["loss_sum"] == 0.0
        if n == 0:
            assert r["last_loss"] == 0.0
        else:
            want = host[:n].astype(np.float64).sum() / n
            assert abs(r["last_loss"] - want) <= 3e-6 * want, (n, r["last_loss"], want)
        slots = ring.cpu().numpy().reshape(16, 2)
        assert tuple(slots[it % 16]) == pairs[it], (it, slots)
    want = [pairs[16], pairs[17]] + pairs[2:16]
    assert [tuple(x) for x in slots] == want


# ---- 10: the deferred update --------------------------------------------------------------------------------------
def test_deferred_update_applies_the_same_values_and_no_bookkeeping(cuda):
    """ngp_fused_optimizer_update: p / m / v (and shadows, gradient) bit for
    bit those of ngp_fused_optimizer_step; end_pending = 1 and every scaler /
    count word untouched (the bookkeeping runs in a later launch, which needs a
    scene: the trainer test below)."""
    case = _case("R4")
    a, b = Dev(case, cuda), Dev(case, cuda)
    sa, sb = State(cuda, case.scale, tracker=2, adam_step=3, epoch=5, iter=5), \
        State(cuda, case.scale, tracker=2, adam_step=3, epoch=5, iter=5)
    a.run(sa, entry="step", iters=8, growth_interval=5)
    b.run(sb, entry="update", iters=8)
    x, y = a.download(), b.download()
    for kind in "pmvgh":
        assert np.array_equal(x[kind], y[kind]), kind
    assert sa.machine_words() == (case.scale, 3, 4, 6, 6)
    r = sb.read()
    assert sb.machine_words() == (case.scale, 2, 3, 5, 5) and r["end_pending"] == 1 and r["found_inf"] == 0
    pairs = oc.one_update(case, adam_step=3, epoch=5, iters=8)
    check_buffers(case, b.host_bits(), y, ref_pairs=pairs, label="R4 deferred, adam_step 3 epoch 5")


# ---- the ABI's rejections -------------------------------------------------------------------------------------------
def test_optimizer_rejects_bad_arguments_before_any_launch(cuda):
    case = _case("R4")
    dev, st = Dev(case, cuda), State(cuda)
    assert dev.launch(st, arrays=dev.arrays(shift=("p", 4))) != 0   # p 4- but not 16-byte aligned
    assert dev.launch(st, arrays=dev.arrays(shift=("v", 8))) != 0
    assert dev.launch(st, arrays=dev.arrays(shift=("g", 2))) != 0   # gradient not 8-byte aligned
    assert dev.launch(st, arrays=(0,) + dev.arrays()[1:]) != 0
    assert dev.launch(st, arrays=dev.arrays(n=9)) != 0
    nat = _nat()
    p = torch.zeros(8, device=cuda)
    assert nat.lib().ngp_adam_step(p.data_ptr(), p.data_ptr(), 0, p.data_ptr(), p.data_ptr(), 8, 1e-2, 0.9, 0.99,
                                   1e-15, 0.0, 0, 1.0, nat.stream_of(p)) != 0  # step 0
    after, host = dev.download(), dev.host_bits()
    assert all(np.array_equal(after[kind], host[kind]) for kind in "pmvgh")  # nothing was launched
    assert st.machine_words() == (65536.0, 0, 0, 0, 0)


# ---- 11: ngp_adam_step ------------------------------------------------------------------------------------------------
def _adam_step_case(cuda, dt, wd, gs, step, n, report=None):
    nat = _nat()
    p, m, v, g = oc.adam_step_inputs(dt, gs, n)
    G = oc.GUARD

    def guarded(a, canary):
        buf = np.full(n + G, canary, a.dtype)
        buf[:n] = a
        return torch.from_numpy(buf).to(cuda), buf
    nan32 = np.array([0x7fc0a005], np.uint32).view(np.float32)[0]
    nan16 = np.array([0x7e33], np.uint16).view(np.float16)[0]
    (tp, hp), (tm, hm), (tv, hv) = (guarded(a, nan32) for a in (p, m, v))
    tg, hg = guarded(g, nan16 if dt == "f16" else nan32)
    rc = nat.lib().ngp_adam_step(tp.data_ptr(), tg.data_ptr(), 1 if dt == "f16" else 0, tm.data_ptr(), tv.data_ptr(),
                                 n, oc.LR, oc.B1, oc.B2, oc.EPS, wd, step, gs, nat.stream_of(tp))
    nat.check(rc, "adam_step")
    torch.cuda.synchronize()
    ref = oc.adam_reference_f64(p, m, v, g, scale=1.0, grad_mult=np.float64(np.float32(gs)), step=step,
                                weight_decay=wd)
    res = oc.adam_step_restated_f32(p, m, v, g, weight_decay=wd, step=step, grad_scale=gs)
    label = f"adam_step {dt} wd {wd} scale {gs:.3g} step {step} n {n}"
    same = []
    for i, (kind, t, h) in enumerate((("p", tp, hp), ("m", tm, hm), ("v", tv, hv))):
        got = t.cpu().numpy()
        assert np.array_equal(_bits(got[n:]), _bits(h[n:])), (label, kind, "canary")
        ok, fig, allowed = oc.within_margin(got[:n], ref[i], oc.error_figures(res[i], ref[i]))
        assert ok, (label, kind, fig, allowed)
        same.append(float((_bits(got[:n]) == _bits(res[i])).mean()))
    assert np.array_equal(_bits(tg.cpu().numpy()), _bits(hg)), (label, "gradient written")
    return same


def test_adam_step_small_shapes(cuda, parity_report):
    """ngp_adam_step against the float64 reference with the margin rule: fp32
    and fp16 gradients, weight decay 0 and 0.01, grad_scale 1 and 1/65536,
    step 1, 2 and 1000, n in {1, 3, 4, 5, 1027} (scalar tails of every length,
    a second trip of one thread), canaries behind every buffer."""
    ADAM_STEP_CASES = oc.ADAM_STEP_CASES
    worst = [1.0, 1.0, 1.0]
    for c in ADAM_STEP_CASES:
        worst = [min(a, b) for a, b in zip(worst, _adam_step_case(cuda, *c))]
    parity_report(f"ngp_adam_step, {len(ADAM_STEP_CASES)} cases: least share bit-identical to the float32 "
                  f"restatement p {worst[0]:.4f} m {worst[1]:.4f} v {worst[2]:.4f}")


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_adam_step_past_the_block_cap(cuda, parity_report, dt):
    """n = 4096 x 256 x 4 + 3: the grid is capped at 4096 blocks, so thread 0
    makes a second trip and it is the 3-value scalar tail."""
    same = _adam_step_case(cuda, dt, 0.01, 1 / 65536, 2, 4096 * 256 * 4 + 3)
    parity_report(f"ngp_adam_step {dt} n 4194307: bit-identical p {same[0]:.4f} m {same[1]:.4f} v {same[2]:.4f}")


# ---- 1 (RBIG) ----------------------------------------------------------------------------------------------------------
def test_one_update_of_rbig(cuda, parity_report, rbig):
    """One clean update of 16 779 267 values: past k_nonfinite's grid and, on
    a 256-CU part, past the Adam grid's cap (every block sweeps several chunks)."""
    case, dev = rbig
    for kind in "pmvgh":
        dev.upload(kind)
    st = State(cuda, case.scale)
    dev.run(st)
    assert st.machine_words() == (case.scale, 1, 1, 1, 1)
    check_buffers(case, dev.host_bits(), dev.download(), ref_pairs=oc.one_update(case), report=parity_report,
                  label="RBIG")


# ---- 12: the schedule through the trainer ---------------------------------------------------------------------------------
STRUCTURES = {"default": {}, "tail_in_fwd=False": {"tail_in_fwd": False}, "emit_inline=False": {"emit_inline": False},
              "march_adam=False": {"march_adam": False}, "split_head=True": {"split_head": True},
              "draw_ahead=False": {"draw_ahead": False}}


def _trainer(cuda, options, **kw):
    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(cuda)
    with torch.no_grad():
        model.encoder.embeddings.normal_(0, 0.05)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield(cascade=model.cascade, bound=1.0)).to(cuda))
    return FusedTrainer(model, SyntheticLego(cuda, num_rays=1024), M=30080, seed=3, options=options, **kw)


def _train_schedule(cuda, options):
    s = oc.SCHEDULE
    ft = _trainer(cuda, options, iters=s["iters"], growth_interval=s["growth_interval"], init_scale=s["init_scale"])
    for it in range(s["K"]):
        ft.step()
        if it in s["inf_updates"]:
            # as a backward kernel would: bit 0 of the found-inf word, after the
            # backward whose update is to be skipped (applied by the next step or the flush)
            ft._state_i()[W_INF] |= 1
    ft.flush()
    torch.cuda.synchronize()
    i = ft._state_i().cpu().numpy()
    words = (float(i.view(np.float32)[W_SCALE]), int(i[W_TRACKER]), int(i[W_ADAM]), int(i[W_EPOCH]), int(i[W_ITER]))
    ck = ft.checkpoint()
    lrs = {g["lr"] for g in ck["optimizer"]["param_groups"]} | set(ck["lr_scheduler"]["_last_lr"])
    return dict(words=words, steps=ft.optimizer_steps, lrs=lrs, lr=ft.lr, found_inf=int(i[W_INF]),
                params=[p.detach().cpu().clone() for p in ft.params], m=ft.exp_avg.cpu().clone(),
                v=ft.exp_avg_sq.cpu().clone())


@functools.lru_cache(maxsize=None)
def _default_schedule(cuda):
    return _train_schedule(cuda, {})


@pytest.mark.parametrize("structure", list(STRUCTURES))
def test_schedule_through_the_trainer(cuda, structure):
    """The schedule through FusedTrainer.step (eager, 1024 rays) in every step
    structure that places the bookkeeping in another launch: the final state
    words equal the machine's, 10 optimizer steps, the checkpoint's LR is
    lr * 0.1 (the clamp), and parameters and moments are bit-equal to the
    default structure's."""
    got = _default_schedule(cuda) if structure == "default" else _train_schedule(cuda, STRUCTURES[structure])
    mach = oc.ScalerMachine(oc.SCHEDULE["init_scale"], growth_interval=oc.SCHEDULE["growth_interval"])
    for it in range(oc.SCHEDULE["K"]):
        mach.update(int(it in oc.SCHEDULE["inf_updates"]))
    assert got["words"] == mach.state() == (16384.0, 2, 10, 14, 14), got["words"]
    assert got["steps"] == 10 and got["found_inf"] == 0
    assert got["lrs"] == {got["lr"] * 0.1}, got["lrs"]
    ref = _default_schedule(cuda)
    for a, b in zip(got["params"], ref["params"]):
        assert torch.equal(a, b)
    assert torch.equal(got["m"], ref["m"]) and torch.equal(got["v"], ref["v"])
    assert all(bool(torch.isfinite(p).all()) for p in got["params"])


# ---- 13: the march launch's sweep on a ragged list ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R8", "R4"])
def test_march_launch_sweep_on_a_ragged_list(cuda, name):
    """adam_sweep_pipe (the Adam waves of the march launch) on R8 / R4: the
    trainer's march + Adam launch takes its tensor list from the job it is
    handed on every eager call, pointed here at the case's buffers. The
    update it applies equals the plain sweep's (ngp_fused_optimizer_update)
    bit for bit, shadows, cleared gradients and canaries included."""
    ft = _trainer(cuda, {})
    assert ft._march_adam
    case = _case(name)
    a, b = Dev(case, cuda), Dev(case, cuda)
    ft._sample()
    n, P, G, M, V, H, sizes = a.arrays()
    job = ft._job
    assert (job.lr, job.iters, job.zero_grads, job.grad_mult) == (np.float32(oc.LR), 30000, 1, 1.0)
    job.n_tensors = n
    for q in range(n):
        job.params[q], job.grads[q], job.exp_avg[q], job.exp_avg_sq[q] = P[q], G[q], M[q], V[q]
        job.half_params[q], job.sizes[q] = H[q], sizes[q]
    ft._march(adam=True)
    st = State(cuda, case.scale)
    b.run(st, entry="update", mode=PRECHECKED)
    x, y = a.download(), b.download()
    for kind in "pmvgh":
        assert np.array_equal(x[kind], y[kind]), (kind, np.flatnonzero(x[kind] != y[kind])[:8])
    check_buffers(case, a.host_bits(), x, ref_pairs=_one_update(name), label=f"{name} march launch")
    i = ft._state_i().cpu().numpy()
    assert (int(i[W_PENDING]), int(i[W_ADAM]), int(i[W_INF])) == (1, 0, 0)
