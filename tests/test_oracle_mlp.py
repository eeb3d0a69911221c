"""The oracle's MLP (oracle.mlp_forward / mlp_backward with their `act` and
`out_act` arguments) against torch autograd in float64, without a GPU.

tests/test_gpu_ffmlp.py takes these functions as the reference of every FFMLP
activation and shape, so they are checked first: each activation's forward
against a plain torch MLP, each "derivative expressed through y" of the
backward against autograd through the function itself, on the three
(in_dim, hidden, num_layers) shapes the GPU cases use, which also pins
mlp_layers' flat weight layout. The range conditions of every GPU case (on the
oracle alone) run here as well.
"""
import numpy as np
import pytest
import torch

import ffmlp_cases as fc
import oracle

SHAPES = [(16, 64, 2), (48, 32, 4), (64, 64, 3)]
B = 11
K = 10.0


def torch_act(a, z):
    if a == 0: return torch.relu(z)
    if a == 1: return torch.exp(z)
    if a == 2: return torch.sin(z)
    if a == 3: return 1 / (1 + torch.exp(-z))
    if a == 4:
        y = z * K
        return 0.5 * (y + torch.sqrt(y * y + 4)) / K
    if a == 5: return torch.log(torch.exp(z * K) + 1) / K
    return z


class SinePassThrough(torch.autograd.Function):
    """sin(z) whose backward hands the delta on unchanged."""

    @staticmethod
    def forward(ctx, z):
        return torch.sin(z)

    @staticmethod
    def backward(ctx, g):
        return g


def torch_mlp(x, w, in_dim, hidden, nl, act, out_act, hidden_fn=None):
    """[hidden, in], (nl - 1) x [hidden, hidden], [16, hidden] row-major
    nn.Linear matrices back to back in the flat vector, split here by hand."""
    shapes = [(hidden, in_dim)] + [(hidden, hidden)] * (nl - 1) + [(fc.OUT, hidden)]
    h, off = x, 0
    for li, (o, i) in enumerate(shapes):
        z = h @ w[off:off + o * i].view(o, i).T
        off += o * i
        if li < len(shapes) - 1:
            h = hidden_fn(z) if hidden_fn else torch_act(act, z)
        else:
            h = torch_act(out_act, z)
    assert off == w.numel()
    return h


def inputs(in_dim, hidden, nl, act, seed):
    rng = np.random.default_rng([seed, in_dim, hidden, nl, act])
    x = rng.standard_normal((B, in_dim)) * 0.5
    s = 0.5 if act == 1 else 1.0  # as the GPU cases: exponential layers grow
    w = rng.uniform(-1, 1, fc.num_params(in_dim, hidden, nl)) * np.sqrt(3 / hidden) * s
    g = rng.standard_normal((B, fc.OUT))
    return x, w, g


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("act", range(7))
def test_forward_hidden_activation(shape, act):
    in_dim, hidden, nl = shape
    x, w, _ = inputs(in_dim, hidden, nl, act, 1)
    out, hs = oracle.mlp_forward(x, w, in_dim, fc.OUT, hidden, nl, act=act, fp16=False)
    assert out.dtype == np.float64 and len(hs) == nl and all(h.shape == (B, hidden) for h in hs)
    ref = torch_mlp(torch.from_numpy(x), torch.from_numpy(w), in_dim, hidden, nl, act, 6)
    np.testing.assert_allclose(out, ref.numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("out_act", range(7))
def test_forward_output_activation(shape, out_act):
    in_dim, hidden, nl = shape
    x, w, _ = inputs(in_dim, hidden, nl, 0, 2)
    out, _ = oracle.mlp_forward(x, w, in_dim, fc.OUT, hidden, nl, act=0, out_act=out_act, fp16=False)
    ref = torch_mlp(torch.from_numpy(x), torch.from_numpy(w), in_dim, hidden, nl, 0, out_act)
    np.testing.assert_allclose(out, ref.numpy(), rtol=1e-12, atol=0)


def test_sigmoid_is_the_function():
    z = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    np.testing.assert_allclose(oracle._act(3, z.numpy()), torch.sigmoid(z).numpy(), rtol=1e-15, atol=0)


def test_softplus_is_the_function():
    """_act(5) is written log(exp(10 z) + 1) / 10; it is torch's softplus with
    beta = 10 up to the rounding of exp(10 z) + 1 (half an ulp of a number in
    [1, 2), over 10) for z <= 0 and the rounding of the result above."""
    z = np.linspace(-8, 8, 4001)
    ref = torch.nn.functional.softplus(torch.from_numpy(z), beta=K, threshold=1e9).numpy()
    np.testing.assert_allclose(oracle._act(5, z), ref, rtol=1e-15, atol=2.0 ** -53 / 10 * 1.01)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("act", [0, 1, 3, 4, 5, 6])
def test_backward_matches_autograd(shape, act):
    """Autograd through the function itself against the oracle's derivative
    expressed through the post-activation y (1 - exp(-10 y) for softplus,
    t^2 / (t^2 + 1) with t = 10 y for squareplus, ...)."""
    in_dim, hidden, nl = shape
    x, w, g = inputs(in_dim, hidden, nl, act, 3)
    gi, gw = oracle.mlp_backward(g, x, w, in_dim, fc.OUT, hidden, nl, act=act, fp16=False)
    xt = torch.from_numpy(x).requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    torch_mlp(xt, wt, in_dim, hidden, nl, act, 6).backward(torch.from_numpy(g))
    np.testing.assert_allclose(gi, xt.grad.numpy(), rtol=1e-9, atol=0)
    np.testing.assert_allclose(gw, wt.grad.numpy(), rtol=1e-9, atol=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_sine_passes_delta_through(shape):
    """The reference leaves the sine backward unwritten (ffmlp/src/utils.h:552-556:
    the case returns without writing the result fragment), so this
    project defines it: the delta passes through the sine layers unchanged
    (act_bwd's default branch in csrc/ffmlp.hip, _act_bwd's in the oracle).
    The grads are those of autograd with d sin / dz replaced by 1, not the
    gradient of the function."""
    in_dim, hidden, nl = shape
    x, w, g = inputs(in_dim, hidden, nl, 2, 4)
    gi, gw = oracle.mlp_backward(g, x, w, in_dim, fc.OUT, hidden, nl, act=2, fp16=False)
    xt = torch.from_numpy(x).requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    torch_mlp(xt, wt, in_dim, hidden, nl, 2, 6, hidden_fn=SinePassThrough.apply).backward(torch.from_numpy(g))
    np.testing.assert_allclose(gi, xt.grad.numpy(), rtol=1e-9, atol=0)
    np.testing.assert_allclose(gw, wt.grad.numpy(), rtol=1e-9, atol=0)
    # and it is not the true gradient
    xt2 = torch.from_numpy(x).requires_grad_(True)
    torch_mlp(xt2, torch.from_numpy(w), in_dim, hidden, nl, 2, 6).backward(torch.from_numpy(g))
    assert not np.allclose(gi, xt2.grad.numpy(), rtol=1e-3)


# ---- the GPU cases' conditions on the oracle alone ---------------------------

@pytest.mark.parametrize("spec,backward", fc.all_cases(),
                         ids=lambda v: "-".join(str(int(e)) for e in v) if isinstance(v, tuple) else str(v))
def test_gpu_case_ranges(spec, backward):
    """Finite oracle values, |z| <= 8, the fp32 formula's own share within the
    cap and its dW inside the 0.9 contract, for every case
    tests/test_gpu_ffmlp.py runs. The batches of a few rows take the output and
    grad_inputs shares over their group's pooled rows, below."""
    fc.get(spec, backward).check_ranges(pooled=spec[3] in fc.B_SMALL)


@pytest.mark.parametrize("act", fc.ACTS_EDGE)
def test_gpu_small_batches(act):
    cases = fc.small_cases(act)
    fc.check_small(cases)
    for c in cases:
        for what in ("out", "gi"):
            # a bound no batch can meet by being wrong everywhere: at most one
            # of the 1-row batch's 16 outputs, three of its 32 input gradients
            assert fc.small_min_equal(cases, c, what) >= (0.87 if c.B == 1 else 0.95), (c.B, what)


def test_wide_cases_reach_far():
    """Case g takes squareplus and softplus to |z| ~ 5, either sign."""
    for a in fc.ACTS_WIDE:
        c = fc.case(*fc.SHAPE_WIDE, fc.B_WIDE, a, wide=True)
        assert c.zmin_hidden <= -4.5 and 4.5 <= c.zmax <= fc.Z_MAX


def test_gpu_cases_cover_every_instantiation():
    """All 12 <W, IN_KS, NH> of MLP_DISPATCH appear among the ReLU cases and the
    generic-activation shapes are among them."""
    inst = {(h, (i + 31) // 32, n - 1) for (i, h, n) in fc.SHAPES_RELU}
    assert inst == {(h, ks, nh) for h in (32, 64) for ks in (1, 2) for nh in (1, 2, 3)}
    assert len(fc.SHAPES_RELU) == 16 and {s for s in fc.SHAPES_ACT} <= set(fc.SHAPES_RELU)
    assert fc.B_FWD_STRIDE > 2048 * 4 * 32 and fc.B_BWD_STRIDE > 256 * 4 * 32
