"""The stand-alone SH encoder (csrc/shencoder.hip, csrc/sh_basis.h) through
`_backend` and the autograd operator, at every degree, in float32 and float64,
on the cases of tests/sh_cases.py.

Values and the saved Jacobian `dy_dx` ([B, 3, C*C]) lie within 4 x base of the
exact polynomials, per column and per radius group, where the base is the
references' own rounding error (sh_cases.references) and 4 is this project's
margin for another operation order, nothing more. Where the base is zero the
kernel is exact. The float64 kernels multiply by float32-rounded literals
(the `...f` of sh_basis.h), so their target is the long-double evaluation with
the same literals.

On the unit group the values also lie within 4 x base + 1e-12 of the
independent recurrence definition. For the float64 kernels that bound carries
one more term, `literal` = max |long-double table with float32-rounded
literals - independent| per column (up to 1.4e-6, references only): their
literals are float32 by design, so they are that far from the definition
before any rounding of their own.

Backward: prefill + sum over the kernel's own dy_dx, read back, within the
bound of a sequential sum of C*C + 1 terms, (C*C + 1) u (|prefill| +
sum |g dd|), u = 2^-24 or 2^-53.
"""
import numpy as np
import pytest
import torch

import oracle
import sh_cases as sc

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, np.float32, 2.0 ** -24), "f64": (torch.float64, np.float64, 2.0 ** -53)}
DEGREES = range(1, 9)
PAD = 3  # canary rows on either side of a buffer


@pytest.fixture(scope="module")
def ref():
    return sc.references()


def _backend():
    from shencoder.backend import _backend as b
    return b


class Guarded:
    """`rows` rows of `width` elements inside a buffer of 0xA5 bytes, PAD
    canary rows before and after. `t` is the contiguous view the kernel gets."""

    def __init__(self, rows, width, tdtype, dev, pad=PAD):
        self.item = torch.empty(0, dtype=tdtype).element_size()
        self.front = pad * max(width, 1)
        self.n = rows * width
        self.raw = torch.full(((2 * self.front + self.n) * self.item,), 0xA5, dtype=torch.uint8, device=dev)
        self.t = self.raw.view(tdtype)[self.front:self.front + self.n]
        assert self.t.is_contiguous() and self.t.numel() == self.n

    def intact(self):
        raw = self.raw.cpu().numpy()
        a, b = self.front * self.item, (self.front + self.n) * self.item
        return bool((raw[:a] == 0xA5).all() and (raw[b:] == 0xA5).all())

    def untouched(self):
        return bool((self.raw.cpu().numpy() == 0xA5).all())

    def numpy(self):
        return self.t.cpu().numpy()


def forward(pts, dtype, degree, dev, with_jac=True):
    """One `_backend.sh_encode_forward` on the test's own guarded buffers.
    Returns (values [B, C2], dy_dx [B, 3, C2] or None, the dy_dx Guarded)."""
    tdtype, ndtype, _ = DTYPES[dtype]
    B, C2 = len(pts), degree * degree
    x = Guarded(B, 3, tdtype, dev)
    x.t.copy_(torch.from_numpy(np.ascontiguousarray(pts, dtype=ndtype).reshape(-1)))
    x_bytes = x.raw.clone()
    out = Guarded(B, C2, tdtype, dev)
    dd = Guarded(B, 3 * C2, tdtype, dev) if with_jac else None
    _backend().sh_encode_forward(x.t, out.t, B, 3, degree, dd.t if with_jac else None)
    torch.cuda.synchronize()
    assert out.intact(), ("outputs canary", dtype, degree, B, with_jac)
    assert torch.equal(x.raw, x_bytes), ("inputs written", dtype, degree, B)
    if with_jac:
        assert dd.intact(), ("dy_dx canary", dtype, degree, B)
    vals = out.numpy().reshape(B, C2)
    return vals, (dd.numpy().reshape(B, 3, C2) if with_jac else None), dd


def value_errors(got, rows, dtype, C2, ref):
    """(|got - target| as float64 [B, C2], 4 x base tolerance [B, C2])."""
    if dtype == "f32":
        err = np.abs(got.astype(np.float64) - ref.val[rows, :C2])
    else:
        err = np.abs(got.astype(np.longdouble) - ref.val_ld[rows, :C2]).astype(np.float64)
    return err, ref.base[dtype, "val"][sc.GROUP_ID[rows], :C2]


def jacobian_errors(got, rows, dtype, C2, ref):
    """(|dy_dx - exact| [B, 3, C2], base [B, 3, C2])."""
    if dtype == "f32":
        err = np.abs(got.astype(np.float64) - ref.jac[rows][:, :, :C2])
    else:
        err = np.abs(got.astype(np.longdouble) - ref.jac_ld[rows][:, :, :C2]).astype(np.float64)
    return err, ref.base[dtype, "jac"][sc.GROUP_ID[rows]][:, :, :C2]


def band_ratios(err, base, degree):
    """Largest err / base per band over the entries whose base is not zero;
    err and base end in the column axis."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(base > 0, err / base, 0.0)
    r = r.reshape(-1, r.shape[-1]).max(0)
    return [float(r[l * l:(l + 1) ** 2].max()) for l in range(degree)]


def check_values(got, rows, dtype, degree, ref, what):
    C2 = degree * degree
    assert got.shape == (len(rows), C2) and np.isfinite(got).all(), what
    err, base = value_errors(got, rows, dtype, C2, ref)
    bad = err > 4 * base
    assert not bad.any(), (what, np.argwhere(bad)[:4], err[bad][:4], base[bad][:4])
    unit = sc.GROUP_ID[rows] == 0
    if unit.any():
        extra = ref.literal[:C2] if dtype == "f64" else 0.0
        e = np.abs(got[unit].astype(np.float64) - ref.indep[rows[unit], :C2])
        tol = 4 * ref.base[dtype, "val"][0, :C2] + 1e-12 + extra
        assert (e <= tol).all(), (what, "independent", np.argwhere(e > tol)[:4])
    return band_ratios(err, base, degree)


def check_jacobian(got, rows, dtype, degree, ref, what):
    C2 = degree * degree
    assert got.shape == (len(rows), 3, C2) and np.isfinite(got).all(), what
    assert (got[:, :, 0] == 0).all(), (what, "column 0")
    err, base = jacobian_errors(got, rows, dtype, C2, ref)
    bad = err > 4 * base
    assert not bad.any(), (what, np.argwhere(bad)[:4], err[bad][:4], base[bad][:4])
    return band_ratios(err, base, degree)


def _fmt(r):
    return " ".join(f"{v:.2f}" for v in r)


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_forward_values_and_canaries(cuda, ref, parity_report, dtype, degree):
    """Every batch size, with and without dy_dx: canary rows intact, values
    within 4 x base of the exact polynomials; the run without dy_dx gives the
    same bits as the run with it."""
    worst = np.zeros(degree)
    for B in sc.BATCHES:
        rows = sc.batch_rows(B)
        with_j, _, _ = forward(ref.pts[rows], dtype, degree, cuda, with_jac=True)
        without, none, _ = forward(ref.pts[rows], dtype, degree, cuda, with_jac=False)
        assert none is None
        assert np.array_equal(with_j.view(np.uint8), without.view(np.uint8)), (dtype, degree, B)
        worst = np.maximum(worst, check_values(with_j, rows, dtype, degree, ref, (dtype, degree, B)))
    line = f"{dtype} degree {degree}: value error / base per band: {_fmt(worst)}"
    print(line)
    if degree in (4, 8):
        parity_report(line)


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_saved_jacobian(cuda, ref, parity_report, dtype, degree):
    """dy_dx entry by entry in its [B, 3, C*C] layout against the exact
    Jacobian (complex step); column 0 exact zeros."""
    worst = np.zeros(degree)
    for B in sc.BATCHES:
        rows = sc.batch_rows(B)
        _, jac, _ = forward(ref.pts[rows], dtype, degree, cuda)
        worst = np.maximum(worst, check_jacobian(jac, rows, dtype, degree, ref, (dtype, degree, B)))
    line = f"{dtype} degree {degree}: dy_dx error / base per band: {_fmt(worst)}"
    print(line)
    if degree in (4, 8):
        parity_report(line)


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_backward_adds_into_grad_inputs(cuda, ref, parity_report, dtype, degree):
    """grad_inputs = prefill + sum_c grad * dy_dx (the reference's `+=`,
    shencoder.cu:358-382) within the sequential-sum bound; the elements past
    B*3 of a longer grad_inputs keep their bits; two runs give the same bits."""
    tdtype, ndtype, u = DTYPES[dtype]
    wide = np.longdouble if dtype == "f64" else np.float64
    C2 = degree * degree
    tail = 67
    worst = 0.0
    for B in sc.BATCHES:
        rows = sc.batch_rows(B)
        _, jac, dd = forward(ref.pts[rows], dtype, degree, cuda)
        rng = np.random.default_rng(1000 * degree + B)
        g = rng.standard_normal((B, C2)).astype(ndtype)
        pre = rng.standard_normal(B * 3 + tail).astype(ndtype)
        grad = Guarded(B, C2, tdtype, cuda)
        grad.t.copy_(torch.from_numpy(g.reshape(-1)))
        x = torch.from_numpy(ref.pts[rows].astype(ndtype)).to(cuda)
        runs = []
        for _ in range(2):
            gi = Guarded(1, B * 3 + tail, tdtype, cuda)
            gi.t.copy_(torch.from_numpy(pre))
            _backend().sh_encode_backward(grad.t, x, B, 3, degree, dd.t, gi.t)
            torch.cuda.synchronize()
            assert gi.intact() and dd.intact() and grad.intact(), (dtype, degree, B)
            runs.append(gi.numpy())
        assert np.array_equal(dd.numpy().reshape(B, 3, C2).view(np.uint8), jac.view(np.uint8))
        assert np.array_equal(runs[0].view(np.uint8), runs[1].view(np.uint8)), (dtype, degree, B)
        got = runs[0]
        assert np.array_equal(got[B * 3:].view(np.uint8), pre[B * 3:].view(np.uint8)), (dtype, degree, B)
        terms = g.astype(wide)[:, None, :] * jac.astype(wide)
        p = pre[:B * 3].astype(wide).reshape(B, 3)
        exact = p + terms.sum(-1)
        bound = ((C2 + 1) * u * (np.abs(p) + np.abs(terms).sum(-1))).astype(np.float64)
        err = np.abs(got[:B * 3].astype(wide).reshape(B, 3) - exact).astype(np.float64)
        assert (bound > 0).all()
        assert (err <= bound).all(), (dtype, degree, B, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    line = f"{dtype} degree {degree}: backward error / derived bound {worst:.3f}"
    print(line)
    if degree in (4, 8):
        parity_report(line)


@pytest.mark.parametrize("degree", [4, 8])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_nan_rows_stay_in_their_row(cuda, ref, dtype, degree):
    """A NaN component makes NaN exactly the columns that the float32 oracle
    makes NaN, column 0 stays the constant, and every other row of outputs
    and dy_dx keeps its bits."""
    B = 65
    rows = sc.batch_rows(B)
    clean = ref.pts[rows].copy()
    dirty = clean.copy()
    hit = {10: 0, 20: 1, 31: 2, 64: 0}            # row -> the component that becomes NaN
    for r, c in hit.items():
        dirty[r, c] = np.nan
    v0, j0, _ = forward(clean, dtype, degree, cuda)
    v1, j1, _ = forward(dirty, dtype, degree, cuda)
    with np.errstate(all="ignore"):
        want = np.isnan(oracle.sh_encode(dirty, degree))
    assert want[list(hit)].any(1).all() and not want[:, 0].any()
    assert np.array_equal(np.isnan(v1), want)
    assert v1[:, 0].tobytes() == v0[:, 0].tobytes()
    keep = np.ones(B, dtype=bool)
    keep[list(hit)] = False
    assert np.array_equal(v1[keep].view(np.uint8), v0[keep].view(np.uint8))
    assert np.array_equal(j1[keep].view(np.uint8), j0[keep].view(np.uint8))
    assert (j1[:, :, 0] == 0).all()


# ------------------------------------------------------- the autograd operator

def test_no_grad_saves_no_jacobian(cuda, ref, monkeypatch):
    import shencoder.sphere_harmonics as mod
    seen = []
    real = mod._backend.sh_encode_forward

    def spy(inputs, outputs, B, D, C, dy_dx):
        seen.append(dy_dx)
        return real(inputs, outputs, B, D, C, dy_dx)
    monkeypatch.setattr(mod._backend, "sh_encode_forward", spy)
    x = torch.from_numpy(ref.pts[sc.batch_rows(65)]).to(cuda)
    enc = mod.SHEncoder(degree=4)
    y = enc(x)
    assert seen[-1] is None and not y.requires_grad
    xr = x.clone().requires_grad_(True)
    y2 = mod.sh_encode(xr, 4, False)
    assert seen[-1] is None
    assert torch.autograd.grad(y2.sum(), xr, allow_unused=True) == (None,)
    y3 = enc(xr)
    assert seen[-1] is not None and seen[-1].shape == (65, 48) and y3.requires_grad
    assert torch.equal(y, y3.detach()) and torch.equal(y, y2.detach())


@pytest.mark.parametrize("degree", [3, 4, 8])
def test_half_inputs_under_autocast(cuda, ref, degree):
    from shencoder import SHEncoder
    enc = SHEncoder(degree=degree)
    x = torch.from_numpy(ref.pts[sc.batch_rows(257)]).to(cuda).half()
    with torch.autocast("cuda", dtype=torch.float16):
        y = enc(x)
    assert y.dtype == torch.float32 and y.shape == (257, degree * degree)
    assert torch.equal(y, enc(x.float()))


@pytest.mark.parametrize("degree", DEGREES)
def test_double_inputs_end_to_end_and_gradcheck(cuda, ref, degree):
    """Double inputs outside autocast take the float64 kernels: the module's
    values and gradient are float64 and within the float64 bounds;
    torch.autograd.gradcheck with its defaults on B = 7."""
    from shencoder import SHEncoder, sh_encode
    C2 = degree * degree
    rows = sc.batch_rows(65)
    x = torch.from_numpy(ref.pts[rows].astype(np.float64)).to(cuda).requires_grad_(True)
    y = SHEncoder(degree=degree)(x)
    assert y.dtype == torch.float64
    check_values(y.detach().cpu().numpy(), rows, "f64", degree, ref, ("module f64", degree))
    g = torch.from_numpy(np.random.default_rng(degree).standard_normal((65, C2))).to(cuda)
    y.backward(g)
    assert x.grad.dtype == torch.float64
    terms = g.cpu().numpy().astype(np.longdouble)[:, None, :] * ref.jac_ld[rows][:, :, :C2]
    # the sum's rounding plus 4 x base of each Jacobian entry it adds up
    base = ref.base["f64", "jac"][sc.GROUP_ID[rows]][:, :, :C2]
    tol = (C2 + 1) * 2.0 ** -53 * np.abs(terms).sum(-1) + (np.abs(g.cpu().numpy())[:, None, :] * 4 * base).sum(-1)
    err = np.abs(x.grad.cpu().numpy().astype(np.longdouble) - terms.sum(-1))
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    x7 = torch.from_numpy(ref.pts[rows[:7]].astype(np.float64)).to(cuda).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: sh_encode(t, degree, True), (x7,))


def test_shapes_sizes_and_the_factory(cuda, ref):
    from encoding import get_encoder
    from shencoder import SHEncoder, sh_encode
    for d in DEGREES:
        enc, dim = get_encoder("sphere_harmonics", degree=d)
        assert isinstance(enc, SHEncoder) and dim == d * d == enc.output_dim and enc.degree == d
    enc = SHEncoder(degree=4)
    rows = sc.batch_rows(63)[:30]       # axes, lattice directions, the zero vector; no denormal
    x = torch.from_numpy(ref.pts[rows]).to(cuda)
    y = enc(x)
    check_values(y.cpu().numpy(), rows, "f32", 4, ref, "module f32")
    # a non-contiguous input
    wide = torch.zeros(30, 6, device=cuda)
    wide[:, ::2] = x
    nc = wide[:, ::2]
    assert not nc.is_contiguous()
    assert torch.equal(enc(nc), y) and torch.equal(sh_encode(nc, 4), y)
    # a [2, 3, 5, 3] prefix shape
    assert torch.equal(enc(x.view(2, 3, 5, 3)), y.view(2, 3, 5, 16))
    # size = 2.0: the encoding of inputs / 2 (a division by two is exact)
    assert torch.equal(enc(x * 2, size=2.0), y)
    # B = 0, forward and backward
    e = torch.empty(0, 3, device=cuda, requires_grad=True)
    z = enc(e)
    assert z.shape == (0, 16) and z.requires_grad
    z.sum().backward()
    assert e.grad.shape == (0, 3)
    assert enc(torch.empty(4, 0, 3, device=cuda)).shape == (4, 0, 16)
    # backward through the non-contiguous, scaled path: d/dx enc(x / 2) = J / 2
    a = nc.clone().requires_grad_(True)
    b = (x * 2).requires_grad_(True)
    g = torch.from_numpy(np.random.default_rng(5).standard_normal((30, 16)).astype(np.float32)).to(cuda)
    enc(a).backward(g)
    enc(b, size=2.0).backward(g)
    assert torch.equal(a.grad * 0.5, b.grad)
    # the operator itself on a non-contiguous input and a non-contiguous grad
    c = wide.clone().requires_grad_(True)
    gw = torch.zeros(30, 32, device=cuda)
    gw[:, ::2] = g
    sh_encode(c[:, ::2], 4, True).backward(gw[:, ::2])
    assert torch.equal(c.grad[:, ::2], a.grad) and float(c.grad[:, 1::2].abs().max()) == 0


# -------------------------------------------------------------------- arguments

def _args(dev, B=5, D=3, C=4, dtype=torch.float32):
    """Guarded buffers of exactly the sizes B, D, C call for."""
    return dict(inputs=Guarded(B, D, dtype, dev), outputs=Guarded(B, C * C, dtype, dev),
                dy_dx=Guarded(B, D * C * C, dtype, dev), grad=Guarded(B, C * C, dtype, dev),
                grad_inputs=Guarded(B, D, dtype, dev))


def _fill(bufs):
    for k in ("inputs", "grad"):
        bufs[k].t.copy_(torch.linspace(-1, 1, bufs[k].n, dtype=bufs[k].t.dtype))
        bufs[k].bytes = bufs[k].raw.clone()


def _all_untouched(bufs):
    torch.cuda.synchronize()
    for k, b in bufs.items():
        if k in ("inputs", "grad"):
            assert torch.equal(b.raw, b.bytes), k
        else:
            assert b.untouched(), k


def _fwd(be, a, B, D, C, **over):
    t = {k: v.t for k, v in a.items()}
    t.update(over)
    be.sh_encode_forward(t["inputs"], t["outputs"], B, D, C, t["dy_dx"])


def _bwd(be, a, B, D, C, **over):
    t = {k: v.t for k, v in a.items()}
    t.update(over)
    be.sh_encode_backward(t["grad"], t["inputs"], B, D, C, t["dy_dx"], t["grad_inputs"])


def test_existing_argument_errors(cuda):
    """D != 3, degree 0, degree 9 and a half tensor raise with the messages
    they always had; the buffers are large enough for each call, so it is the
    argument that is refused. Nothing is written."""
    be = _backend()
    a = _args(cuda, B=5, D=4, C=9)
    _fill(a)
    for D, C, msg in ((2, 4, "input dim == 3"), (4, 4, "input dim == 3"),
                      (3, 0, r"degree in \[1, 8\]"), (3, 9, r"degree in \[1, 8\]")):
        with pytest.raises(RuntimeError, match=msg):
            _fwd(be, a, 5, D, C)
        with pytest.raises(RuntimeError, match=msg):
            _bwd(be, a, 5, D, C)
    h = {k: torch.zeros(5 * 3 * 81, dtype=torch.float16, device=cuda) for k in a}
    for k in ("inputs", "outputs", "dy_dx"):
        with pytest.raises(RuntimeError, match=f"{k} must be a float32/float64 tensor"):
            _fwd(be, a, 5, 3, 4, **{k: h[k]})
    for k in ("grad", "inputs", "dy_dx", "grad_inputs"):
        with pytest.raises(RuntimeError, match=f"{k} must be a float32/float64 tensor"):
            _bwd(be, a, 5, 3, 4, **{k: h[k]})
    with pytest.raises(RuntimeError, match="contiguous"):
        _fwd(be, a, 5, 3, 4, outputs=torch.zeros(5, 32, device=cuda)[:, ::2])
    with pytest.raises(RuntimeError, match="CUDA"):
        _fwd(be, a, 5, 3, 4, inputs=torch.zeros(5, 3))
    _all_untouched(a)
    assert all(float(v.abs().max()) == 0 for v in h.values())


@pytest.mark.parametrize("base_dtype", [torch.float32, torch.float64])
def test_mismatched_tensors_are_refused_before_any_launch(cuda, base_dtype):
    """Tensors of two dtypes, or smaller than B, D, C call for, raise a
    RuntimeError that names the tensor, and no buffer is written: float64
    inputs with a float32 `outputs` of the right shape used to write 8-byte
    values through the 4-byte buffer."""
    be = _backend()
    other = torch.float64 if base_dtype == torch.float32 else torch.float32
    B, C = 5, 4
    a = _args(cuda, B=B, C=C, dtype=base_dtype)
    o = _args(cuda, B=B, C=C, dtype=other)
    _fill(a)
    _fill(o)
    for k in ("outputs", "dy_dx"):
        with pytest.raises(RuntimeError, match=rf"sh_encode_forward: {k} is torch\.float"):
            _fwd(be, a, B, 3, C, **{k: o[k].t})
    with pytest.raises(RuntimeError, match=r"sh_encode_forward: outputs is torch\.float"):
        _fwd(be, o, B, 3, C, inputs=a["inputs"].t)
    for k in ("inputs", "dy_dx", "grad_inputs"):
        with pytest.raises(RuntimeError, match=rf"sh_encode_backward: {k} is torch\.float"):
            _bwd(be, a, B, 3, C, **{k: o[k].t})
    # one row short
    s = _args(cuda, B=B - 1, C=C, dtype=base_dtype)
    _fill(s)
    for k in ("inputs", "outputs", "dy_dx"):
        with pytest.raises(RuntimeError, match=rf"sh_encode_forward: {k} has \d+ elements"):
            _fwd(be, a, B, 3, C, **{k: s[k].t})
    for k in ("grad", "inputs", "dy_dx", "grad_inputs"):
        with pytest.raises(RuntimeError, match=rf"sh_encode_backward: {k} has \d+ elements"):
            _bwd(be, a, B, 3, C, **{k: s[k].t})
    # the right size for degree 4 is too small for degree 5; a negative B
    with pytest.raises(RuntimeError, match="outputs has 80 elements"):
        _fwd(be, a, B, 3, 5)
    with pytest.raises(RuntimeError, match="B must be a non-negative int"):
        _fwd(be, a, -1, 3, C)
    with pytest.raises(RuntimeError, match="B must be a non-negative int"):
        _bwd(be, a, -1, 3, C)
    for bufs in (a, o, s):
        _all_untouched(bufs)
    # and the same buffers, matched, are accepted
    _fwd(be, a, B, 3, C)
    _bwd(be, a, B, 3, C)
    torch.cuda.synchronize()
    assert all(b.intact() for b in a.values())
    assert np.isfinite(a["grad_inputs"].numpy()).all()


class _Elsewhere:
    """Stands in for a tensor on a second GPU (the suite runs on one): all
    that the argument check reads before it refuses, and no data pointer, so
    it cannot reach a launch."""

    def __init__(self, like):
        self.is_cuda, self.dtype, self._n = True, like.dtype, like.numel()
        self.device = torch.device("cuda", like.device.index + 1)

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n


def test_tensors_on_two_devices_are_refused(cuda):
    be = _backend()
    a = _args(cuda)
    _fill(a)
    for k in ("outputs", "dy_dx"):
        with pytest.raises(RuntimeError, match=f"sh_encode_forward: {k} is on cuda:1 but inputs is on cuda:0"):
            _fwd(be, a, 5, 3, 4, **{k: _Elsewhere(a[k].t)})
    for k in ("inputs", "dy_dx", "grad_inputs"):
        with pytest.raises(RuntimeError, match=f"sh_encode_backward: {k} is on cuda:1 but grad is on cuda:0"):
            _bwd(be, a, 5, 3, 4, **{k: _Elsewhere(a[k].t)})
    _all_untouched(a)
