"""GPU: the grid encoder's kernels on inputs whose sums are exact, and on the
dispatch routes no other test takes (tests/grid_cases.py holds the tables,
tests/test_grid_cases_cpu.py proves the inputs' conditions on the CPU).

Backward: on the exact-sum inputs every partial sum, in any order and any
grouping, is an fp16 number, so the fused (binned) backward in each of its
configurations and the generic kernel in each type must give the float64
scatter BIT FOR BIT: one dropped, doubled or misrouted contribution changes
an entry by a multiple of 2^-9 and fails, whichever route made it.

Forward: bit-exact against the oracle for every level count up to 64 (more
than one level group per XCD), every (D, C), the group-major route (2^22
rows), the large-batch grid sized for chunk lending when nothing is lent, and
the rows at the box's faces. NaN coordinates are excluded: the kernel's
`(uint32_t)floorf(NaN)` and the C oracle's are both implementation-defined.
"""
import ctypes

import numpy as np
import pytest
import torch

import grid_cases as gc
import oracle

pytestmark = pytest.mark.gpu

TDT = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
ZEROED, EXTERNAL = 0x10, 0x20  # NGP_GRID_GRAD_ZEROED, NGP_GRID_CURSORS_EXTERNAL
NGP_ERR_ARG = -1


def _nat():
    import _ngp_native as nat
    return nat


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a copy: the shared case data is read-only)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def _S(scale):
    return float(np.float32(np.log2(scale)))


class FusedBackward:
    """ngp_grid_encode_backward_fused on one shape: the workspace is allocated
    once and must come back with its counters cleared after every call."""

    def __init__(self, dev, offs, B, D, C, L, H, scale):
        self.nat, self.dev, self.B, self.D, self.C, self.L, self.H, self.S = _nat(), dev, B, D, C, L, H, _S(scale)
        self.offs_host = np.ascontiguousarray(offs, dtype=np.int32)
        self.hp = self.offs_host.ctypes.data_as(ctypes.c_void_p)
        lib = self.nat.lib()
        nbytes = int(lib.ngp_grid_encode_backward_fused_workspace_bytes(B, D, C, L, self.S, H, 0, self.hp))
        self.cbytes = int(lib.ngp_grid_encode_backward_fused_counter_bytes(B, D, C, L, self.S, H, 0, self.hp))
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev) if nbytes and D == 3 else None
        self.offs = _dev(self.offs_host, dev)

    def __call__(self, g16, w, bound, count=None, layout=1, flags=0, reps=1, flag=None):
        nat, B, L, C = self.nat, self.B, self.L, self.C
        table = torch.zeros(int(self.offs_host[-1]), C, dtype=torch.float16, device=self.dev)
        gt, wt = _dev(g16, self.dev), _dev(w, self.dev)
        if layout == 0:  # [L, B, C]
            gt = gt.view(B, L, C).permute(1, 0, 2).contiguous()
        cnt = torch.tensor([count], dtype=torch.int32, device=self.dev) if count is not None else None
        for _ in range(reps):
            nat.check(nat.lib().ngp_grid_encode_backward_fused(
                nat.ptr(gt), nat.ptr(wt), float(bound), nat.ptr(self.offs), nat.ptr(table), B, nat.ptr(cnt), self.D, C,
                L, self.S, self.H, 0, 0, 0, self.hp, nat.ptr(self.ws), self.ws.numel() if self.ws is not None else 0,
                layout | flags, nat.ptr(flag), nat.stream_of(table)), "grid_backward_fused")
            if flags & EXTERNAL and self.ws is not None:
                self.ws[:self.cbytes].zero_()
        torch.cuda.synchronize()
        if self.ws is not None:  # the bin cursors are left zeroed for the next call
            assert int(self.ws[:self.cbytes - 512].sum()) == 0
        return table.cpu().numpy()


def _mismatch(got, want, offs):
    ne = (_bits(got) != _bits(want)).any(1)
    rows = np.flatnonzero(ne)[:4]
    return (int(ne.sum()), [(int(r), int(np.searchsorted(offs, r, "right") - 1), got[r].tolist(), want[r].tolist())
                            for r in rows])


# ---- A. exact sums --------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in gc.FUSED_EXACT])
def test_fused_backward_exact_sums(cuda, parity_report, name):
    """ngp_grid_encode_backward_fused on the exact-sum inputs: plain (read-
    modify-write), a zeroed grad (stores), and a zeroed grad with the caller
    clearing the cursors (the hashed levels' bins one per wave), both grad
    layouts: the fp16 table is the float64 scatter bit for bit and the
    nonfinite flag stays 0. Cases: a count ending mid-block with bound 2, two
    accumulating calls, 2^22-entry levels, the atomic suffix at 2^23, and 40
    dense levels (levels 32..39 binned with the run merge on: the plan's
    64-bit merge mask)."""
    case, d = gc.EXACT[name], gc.exact_data(name)
    want = d["ref"].astype(np.float16)
    w = gc.world(d["x"], case.bound)
    run = FusedBackward(cuda, d["offs"], case.B, 3, 2, case.L, case.H, case.scale)
    configs = [("plain", 0)] if case.reps > 1 else [("plain", 0), ("zeroed", ZEROED), ("waves", ZEROED | EXTERNAL)]
    for what, flags in configs:
        for layout in (1, 0):
            flag = torch.zeros(1, dtype=torch.int32, device=cuda)
            got = run(d["gd"], w, case.bound, count=case.count, layout=layout, flags=flags, reps=case.reps, flag=flag)
            assert np.array_equal(_bits(got), _bits(want)), (what, layout) + _mismatch(got, want, d["offs"])
            assert int(flag.item()) == 0, (what, layout)
    parity_report(f"{name}: B {case.B} live {case.n} L {case.L} T 2^{case.log2T}: {len(configs) * 2} runs bit-exact, "
                  f"{int((want != 0).any(1).sum())} nonzero entries, max|ref| {float(np.abs(d['ref']).max()):.4g}")


@pytest.mark.parametrize("name", [c.name for c in gc.GENERIC_EXACT])
def test_generic_backward_exact_sums(cuda, name):
    """ngp_grid_encode_backward (k_grid_bwd: corner pairs, the segmented run
    merge) in fp16, fp32 and fp64, every C, D 2..5, both grad layouts, on
    exact-sum inputs with runs of 1, 2, 3, 31, 32, 33 and 70 rows from lane
    0/1 and up to lanes 62/63, an outside row inside a run and cells that share
    a hashed entry: the grad table is the float64 scatter bit for bit."""
    nat = _nat()
    case, d = gc.EXACT[name], gc.exact_data(name)
    dt = np.dtype(case.dtype)
    want = d["ref"].astype(dt)
    B, D, C, L = case.B, case.D, case.C, case.L
    xt, ot = _dev(d["x"], cuda), _dev(d["offs"], cuda)
    for layout in (1, 0):
        g = d["gd"] if layout else np.ascontiguousarray(d["gd"].reshape(B, L, C).transpose(1, 0, 2))
        gt = _dev(g, cuda)
        table = torch.zeros(int(d["offs"][-1]), C, dtype=TDT[dt], device=cuda)
        nat.check(nat.lib().ngp_grid_encode_backward(
            nat.ptr(gt), nat.ptr(xt), None, nat.ptr(ot), nat.ptr(table), B, D, C, L, _S(case.scale), case.H, None,
            None, 0, 0, 0, nat.DTYPE_CODE[TDT[dt]], layout, nat.stream_of(table)), "grid_backward")
        got = table.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (layout,) + _mismatch(got, want, d["offs"])


# ---- C. forward routes ------------------------------------------------------------

def _forward(dev, x, emb, offs, D, C, L, H, scale, layout, dy=False, gridtype=0, ac=0, interp=0):
    """ngp_grid_encode_forward; returns outputs as [B, L*C] (and dy_dx)."""
    nat = _nat()
    B = x.shape[0]
    tdt = TDT[emb.dtype]
    out = torch.full((B, L * C), 7.0, dtype=tdt, device=dev)
    dyt = torch.empty(B, L * D * C, dtype=tdt, device=dev) if dy else None
    xt, et, ot = _dev(x, dev), _dev(emb, dev), _dev(offs, dev)
    rc = nat.lib().ngp_grid_encode_forward(nat.ptr(xt), nat.ptr(et), nat.ptr(ot), nat.ptr(out), B, D, C, L, _S(scale),
                                           H, nat.ptr(dyt), gridtype, ac, interp, nat.DTYPE_CODE[tdt], layout,
                                           nat.stream_of(out))
    nat.check(rc, "grid_forward")
    torch.cuda.synchronize()
    got = out if layout else out.view(L, B, C).permute(1, 0, 2).reshape(B, L * C)
    return got.cpu().numpy(), (dyt.cpu().numpy() if dy else None)


def _forward_fused(dev, w, bound, emb_t, offs_t, B, D, C, L, H, scale, layout, count=None, out=None, gridtype=0,
                   ac=0, interp=0):
    """ngp_grid_encode_forward_fused into a canary-filled fp16 buffer; returns the tensor as [B, L*C]."""
    nat = _nat()
    if out is None:
        out = torch.full((B, L * C), 7.0, dtype=torch.float16, device=dev)
    cnt = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    nat.check(nat.lib().ngp_grid_encode_forward_fused(
        nat.ptr(w), float(bound), nat.ptr(emb_t), nat.DTYPE_CODE[emb_t.dtype], nat.ptr(offs_t), nat.ptr(out), B,
        nat.ptr(cnt), D, C, L, _S(scale), H, gridtype, ac, interp, layout, nat.stream_of(out)), "grid_forward_fused")
    torch.cuda.synchronize()
    return out if layout else out.view(L, B, C).permute(1, 0, 2).reshape(B, L * C)


def _normalise(w, bound):
    return ((w + np.float32(bound)) * np.float32(1.0 / (2.0 * bound))).astype(np.float32)


@pytest.mark.parametrize("L", gc.LEVEL_COUNTS)
def test_forward_level_counts_bit_exact(cuda, L):
    """1..64 levels (more than 16: several level groups per XCD in
    k_grid_fwd_pair), B 129 and 300, both layouts; fp16 and fp32 through
    ngp_grid_encode_forward without dy_dx, and the fused entry on an fp32 table
    read as half and on an fp16 table: bit-exact vs the oracle, the edge rows
    (0, -0.0, 1, the floats next to 0 and 1) and lattice rows included."""
    D, C, H, scale, log2T = 3, 2, 2, 1.1, 8
    offs, emb = gc.forward_table(D, L, C, H, scale, log2T, seed=L)
    for B in (129, 300):
        x = gc.forward_inputs(B, D, seed=B + L)
        w = gc.world(x, 1.0)
        w[-4:, 0] = [1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2))]
        xn = _normalise(w, 1.0)
        ref = {dt: oracle.grid_encode_forward(x, emb.astype(dt), offs, scale, H)[0] for dt in (np.float16, np.float32)}
        ref_fused = oracle.grid_encode_forward(xn, emb.astype(np.float16), offs, scale, H)[0]
        wt, ot = _dev(w, cuda), _dev(offs, cuda)
        for layout in (1, 0):
            for dt in (np.float16, np.float32):
                got, _ = _forward(cuda, x, emb.astype(dt), offs, D, C, L, H, scale, layout)
                assert np.array_equal(_bits(got), _bits(ref[dt])), (B, layout, dt.__name__)
            for et in (_dev(emb, cuda), _dev(emb.astype(np.float16), cuda)):
                got = _forward_fused(cuda, wt, 1.0, et, ot, B, D, C, L, H, scale, layout).cpu().numpy()
                assert np.array_equal(_bits(got), _bits(ref_fused)), (B, layout, str(et.dtype))


def test_forward_rejects_65_levels(cuda):
    nat = _nat()
    D, C, H, scale = 3, 2, 2, 1.05
    offs, emb = gc.forward_table(D, 65, C, H, scale, 8, seed=0)
    x = gc.forward_inputs(129, D, seed=0)
    out = torch.zeros(129, 65 * C, device=cuda)
    xt, et, ot = _dev(x, cuda), _dev(emb, cuda), _dev(offs, cuda)
    args = (nat.ptr(et), nat.ptr(ot), nat.ptr(out), 129, D, C, 65, _S(scale), H)
    assert nat.lib().ngp_grid_encode_forward(nat.ptr(xt), *args, None, 0, 0, 0, 0, 1, nat.stream_of(out)) == NGP_ERR_ARG
    assert nat.lib().ngp_grid_encode_forward_fused(nat.ptr(xt), 1.0, args[0], 0, args[1], args[2], 129, None, D, C, 65,
                                                   _S(scale), H, 0, 0, 0, 1, nat.stream_of(out)) == NGP_ERR_ARG
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # nothing ran


@pytest.mark.parametrize("case", gc.DIM_CASES, ids=lambda c: f"D{c[0]}C{c[1]}t{c[2]}a{c[3]}i{c[4]}")
def test_forward_dims_channels_bit_exact(cuda, case):
    """Every (D, C) in {2..5} x {1, 2, 4, 8}, gridtype / align_corners / interp
    spread over the table: with dy_dx (k_grid_fwd, fp16 / fp32 / fp64) and
    without (k_grid_fwd_pair, fp16 / fp32), both layouts, bit-exact outputs;
    dy_dx within the existing forward test's tolerances."""
    D, C, gt, ac, interp = case
    L, H, scale, log2T, B = 4, 4, 2.0, 10, 300
    offs, emb = gc.forward_table(D, L, C, H, scale, log2T, seed=D * 8 + C, align_corners=bool(ac))
    x = gc.forward_inputs(B, D, seed=D + C, nlat=5 if D < 4 else 3)
    kw = dict(gridtype=gt, ac=ac, interp=interp)
    for dt in (np.float16, np.float32, np.float64):
        ref, ref_dy = oracle.grid_encode_forward(x, emb.astype(dt), offs, scale, H, calc_dy_dx=True, gridtype=gt,
                                                 align_corners=bool(ac), interp=interp)
        for layout in (1, 0):
            got, dy = _forward(cuda, x, emb.astype(dt), offs, D, C, L, H, scale, layout, dy=True, **kw)
            assert np.array_equal(_bits(got), _bits(ref)), ("dy", dt.__name__, layout)
            np.testing.assert_allclose(dy.astype(np.float64), ref_dy.astype(np.float64),
                                       rtol=1e-5 if dt != np.float16 else 2e-3, atol=1e-6 if dt != np.float16 else 2e-3)
            if dt != np.float64:
                got, _ = _forward(cuda, x, emb.astype(dt), offs, D, C, L, H, scale, layout, **kw)
                assert np.array_equal(_bits(got), _bits(ref)), ("pair", dt.__name__, layout)


@pytest.mark.parametrize("D,C", [(2, 4), (4, 1)])
def test_forward_fused_other_dims_bit_exact(cuda, D, C):
    """The fused entry beyond D 3, C 2 (in-kernel normalisation and the row
    count over the generic pair kernel): bound 2, a count, both layouts, an
    fp32 table read as half."""
    L, H, scale, B, n, bound = 5, 4, 2.0, 300, 211, 2.0
    offs, emb = gc.forward_table(D, L, C, H, scale, 10, seed=D + C)
    w = gc.world(gc.forward_inputs(B, D, seed=3, nlat=5 if D < 4 else 3), bound)
    w[-2:, 0] = [bound, np.nextafter(np.float32(bound), np.float32(3))]
    ref = oracle.grid_encode_forward(_normalise(w[:n], bound), emb.astype(np.float16), offs, scale, H)[0]
    wt, et, ot = _dev(w, cuda), _dev(emb, cuda), _dev(offs, cuda)
    for layout in (1, 0):
        got = _forward_fused(cuda, wt, bound, et, ot, B, D, C, L, H, scale, layout, count=n).cpu().numpy()
        assert np.array_equal(_bits(got[:n]), _bits(ref)), layout
        assert np.all(got[n:] == 7.0)


@pytest.mark.parametrize("count", [None, (1 << 22) - 300])
def test_forward_group_major_bit_exact(cuda, count):
    """B = 2^22 + 77 (>= kFwdGroupMajorMin): one level per block, level groups
    outermost. The forward is pointwise, so the oracle runs on the first 256
    rows, the last 400 live rows and 30 000 random rows; the whole output is
    compared bitwise with the same points encoded by two calls below 2^22; rows
    past the count keep their canary."""
    D, C, L, H, scale, log2T = 3, 2, 9, 4, 1.5, 12
    B = (1 << 22) + 77
    n = B if count is None else count
    assert n % 128 != 0
    offs, emb = gc.forward_table(D, L, C, H, scale, log2T, seed=9)
    et, ot = _dev(emb.astype(np.float16), cuda), _dev(offs, cuda)
    gen = torch.Generator(device=cuda)
    gen.manual_seed(22)
    w = torch.rand(B, 3, device=cuda, generator=gen) * 2 - 1
    w[:4] = torch.tensor([[1.5, 0, 0], [1, 1, 1], [-1, -1, -1], [0, -1.0001, 0]], device=cuda)
    out = _forward_fused(cuda, w, 1.0, et, ot, B, D, C, L, H, scale, 1, count=count)
    rows = np.unique(np.r_[np.arange(256), np.arange(n - 400, n),
                           np.random.default_rng(1).integers(0, n, 30000)])
    ws = w[torch.from_numpy(rows).to(cuda)].cpu().numpy()
    ref = oracle.grid_encode_forward(_normalise(ws, 1.0), emb.astype(np.float16), offs, scale, H)[0]
    got = out[torch.from_numpy(rows).to(cuda)].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(ref))
    assert bool((out[n:] == 7.0).all())
    half = 1 << 21
    two = torch.full((B, L * C), 7.0, dtype=torch.float16, device=cuda)
    _forward_fused(cuda, w[:half], 1.0, et, ot, half, D, C, L, H, scale, 1, count=min(n, half), out=two[:half])
    _forward_fused(cuda, w[half:], 1.0, et, ot, B - half, D, C, L, H, scale, 1, count=n - half, out=two[half:])
    assert torch.equal(out.view(torch.int16), two.view(torch.int16))


BORROW_SHAPES = {"bound16": (1.6625, 19), "lego_T14": (gc.LEGO_SCALE, 14)}


@pytest.mark.parametrize("shape,count", [("bound16", None), ("lego_T14", None), ("lego_T14", 0), ("lego_T14", 1),
                                         ("lego_T14", 127), ("lego_T14", 896), ("lego_T14", 1 << 18)])
def test_forward_borrow_grid_without_lending_bit_exact(cuda, shape, count):
    """L 16, B = 2^18: the grid carries the blocks sized for chunk lending, but
    with 4 (a bound-16 model's scale) or 2 (a 2^14 table) dense levels among
    0..7 instead of 5 the device lends nothing and those blocks must do
    nothing. Bit-exact vs the oracle on the first and last 300 live rows and
    40 000 random ones, the whole output equal to two calls of 2^17 rows (below
    the threshold), canaries past the count; counts 0, 1, 127, 896 (the first
    whose 15 % share of live chunks would lend one) and 2^18."""
    scale, log2T = BORROW_SHAPES[shape]
    D, C, L, H, B = 3, 2, 16, 16, 1 << 18
    n = B if count is None else count
    offs, emb = gc.forward_table(D, L, C, H, scale, log2T, seed=3)
    et, ot = _dev(emb.astype(np.float16), cuda), _dev(offs, cuda)
    w = gc.world(gc.forward_inputs(B, D, seed=18), 1.0)
    wt = _dev(w, cuda)
    out = _forward_fused(cuda, wt, 1.0, et, ot, B, D, C, L, H, scale, 1, count=count)
    assert bool((out[n:] == 7.0).all())
    if n:
        rows = np.unique(np.r_[np.arange(min(n, 300)), np.arange(max(n - 300, 0), n),
                               np.random.default_rng(2).integers(0, n, min(n, 40000))])
        ref = oracle.grid_encode_forward(_normalise(w[rows], 1.0), emb.astype(np.float16), offs, scale, H)[0]
        got = out[torch.from_numpy(rows).to(cuda)].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(ref))
    half = B // 2
    two = torch.full((B, L * C), 7.0, dtype=torch.float16, device=cuda)
    _forward_fused(cuda, wt[:half], 1.0, et, ot, half, D, C, L, H, scale, 1, count=min(n, half), out=two[:half])
    _forward_fused(cuda, wt[half:], 1.0, et, ot, half, D, C, L, H, scale, 1, count=max(n - half, 0), out=two[half:])
    assert torch.equal(out.view(torch.int16), two.view(torch.int16))


# ---- D. small gaps ------------------------------------------------------------------

@pytest.mark.parametrize("D,C,dt,layout,interp", [(2, 1, np.float64, 0, 1), (4, 4, np.float64, 1, 0),
                                                  (5, 8, np.float64, 0, 1), (2, 8, np.float16, 0, 1),
                                                  (4, 1, np.float16, 0, 0), (5, 4, np.float16, 1, 1)])
def test_grid_input_backward_dims(cuda, parity_report, D, C, dt, layout, interp):
    """k_grid_input_bwd beyond D 3, C 2, fp32, [B, L*C]: against
    oracle.grid_input_backward on the oracle's own dy_dx, fp64 with the
    tolerances of test_grid_input_backward; fp16 against the float64 result
    within 4x the error the oracle's own fp16 evaluation has against it."""
    nat = _nat()
    L, H, scale, B = 4, 4, 1.6, 300
    offs, emb = gc.forward_table(D, L, C, H, scale, 10, seed=D + C)
    rng = np.random.default_rng(D * 10 + C)
    x = rng.random((B, D), dtype=np.float32)
    _, dy = oracle.grid_encode_forward(x, emb.astype(dt), offs, scale, H, calc_dy_dx=True, interp=interp)
    grad = rng.standard_normal((B, L * C)).astype(dt)
    g_in = grad if layout else np.ascontiguousarray(grad.reshape(B, L, C).transpose(1, 0, 2))
    ref = oracle.grid_input_backward(g_in, dy, B, D, C, L, grad_layout=layout)
    gi = torch.full((B, D), 7.0, dtype=TDT[np.dtype(dt)], device=cuda)
    gemb = torch.zeros(int(offs[-1]), C, dtype=TDT[np.dtype(dt)], device=cuda)
    gt, xt, ot, dyt = _dev(g_in, cuda), _dev(x, cuda), _dev(offs, cuda), _dev(dy, cuda)
    nat.check(nat.lib().ngp_grid_encode_backward(
        nat.ptr(gt), nat.ptr(xt), None, nat.ptr(ot), nat.ptr(gemb), B, D, C, L, _S(scale), H, nat.ptr(dyt),
        nat.ptr(gi), 0, 0, interp, nat.DTYPE_CODE[TDT[np.dtype(dt)]], layout, nat.stream_of(gi)), "grid_backward")
    got = gi.cpu().numpy().astype(np.float64)
    if dt == np.float64:
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5)
        parity_report(f"input backward D{D} C{C} f64 layout {layout}: max err {np.abs(got - ref).max():.3g}")
    else:
        exact = oracle.grid_input_backward(g_in.astype(np.float64), dy.astype(np.float64), B, D, C, L,
                                           grad_layout=layout)
        own = float(np.abs(ref.astype(np.float64) - exact).max())
        err = float(np.abs(got - exact).max())
        parity_report(f"input backward D{D} C{C} f16 layout {layout}: max err {err:.3g}, the oracle's own fp16 "
                      f"evaluation {own:.3g} (allowed 4x)")
        assert own > 0 and err <= 4 * own, (err, own)


@pytest.mark.parametrize("D,C", [(4, 8), (5, 1), (2, 4)])
def test_grad_total_variation_dims(cuda, D, C):
    """k_grid_tv at D 4, D 5 and C 8 / 4, with test_grad_total_variation's tolerances."""
    nat = _nat()
    L, H, scale, log2T, B = 5, 4, 1.6, 12, 4000
    offs, emb = gc.forward_table(D, L, C, H, scale, log2T, seed=D + C)
    rng = np.random.default_rng(12)
    x = rng.random((B, D), dtype=np.float32)
    x[:3] = [[-1e-3] + [0.5] * (D - 1), [1.0] * D, [0.0] * D]
    ref = oracle.grad_total_variation(x, emb, offs, 1e-4, scale, H, 0, False)
    base = (rng.standard_normal(emb.shape) * 1e-6).astype(np.float32)
    grad = _dev(base, cuda)
    xt, et, ot = _dev(x, cuda), _dev(emb, cuda), _dev(offs, cuda)
    nat.check(nat.lib().ngp_grad_total_variation(nat.ptr(xt), nat.ptr(et), nat.ptr(grad), nat.ptr(ot), 1e-4, B, D, C,
                                                 L, _S(scale), H, 0, 0, nat.DTYPE_CODE[torch.float32],
                                                 nat.stream_of(grad)), "grad_tv")
    got = grad.cpu().numpy().astype(np.float64) - base.astype(np.float64)
    assert np.abs(ref).max() > 0 and (ref != 0).sum() > 1000
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())


def test_fused_backward_other_dims_and_nonfinite(cuda, parity_report):
    """ngp_grid_encode_backward_fused at D 2, C 4 (no binned plan: the generic
    kernel over world coordinates and a count, then k_flag_nonfinite over the
    whole table): against the float64 scatter within 2^-8 of each entry's sum
    of |terms|; the flag is 0 on finite input and 1 with one inf grad."""
    D, C, L, H, scale, B, n, bound = 2, 4, 5, 4, 2.0, 3000, 2777, 2.0
    offs = oracle.grid_offsets(D, L, C, H, scale, 10)
    rng = np.random.default_rng(6)
    w = gc.world(rng.random((B, D), dtype=np.float32), bound)
    w[:2] = [[bound * 1.01, 0.0], [0.0, -bound * 1.2]]
    g16 = (rng.standard_normal((B, L * C)) * 0.5).astype(np.float16)
    x = _normalise(w[:n], bound)
    ref = oracle.grid_encode_backward(g16[:n].astype(np.float64), x, offs, C, scale, H)
    mag = oracle.grid_encode_backward(np.abs(g16[:n].astype(np.float64)), x, offs, C, scale, H)
    run = FusedBackward(cuda, offs, B, D, C, L, H, scale)
    for layout in (1, 0):
        flag = torch.zeros(1, dtype=torch.int32, device=cuda)
        got = run(g16, w, bound, count=n, layout=layout, flag=flag).astype(np.float64)
        err = np.abs(got - ref)
        assert (err <= 2.0 ** -8 * mag + 1e-7).all(), float((err / np.maximum(mag, 1e-30)).max())
        assert (ref != 0).sum() > 1000 and int(flag.item()) == 0
    parity_report(f"fused backward D2 C4: worst err / (2^-8 mag + 1e-7) {float((err / (2.0 ** -8 * mag + 1e-7)).max()):.3f}")
    g = g16.copy()
    g[n - 1, 7] = np.float16(np.inf)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda)
    run(g, w, bound, count=n, flag=flag)
    assert int(flag.item()) == 1
    g[n - 1, 7] = 0.5
    g[n, 7] = np.float16(np.inf)  # past the count: not read
    flag.zero_()
    run(g, w, bound, count=n, flag=flag)
    assert int(flag.item()) == 0
