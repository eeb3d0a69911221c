"""Inputs, float64-oracle references and CPU-side bounds of the FFMLP cases
(tests/test_gpu_ffmlp.py runs them on the device, tests/test_oracle_mlp.py
checks the range conditions and the allowances without one).

Everything here is numpy on the CPU: seeded inputs, the oracle's results with
fp16 storage, the range assertions every case has to meet before the device is
touched, and the share of fp16 values that an fp32 evaluation of the same
formulas already costs against the float64 oracle (the basis of the
bit-identical allowance of the non-ReLU activations).
"""
import functools

import numpy as np

import oracle

ACT_NAMES = ["relu", "exponential", "sine", "sigmoid", "squareplus", "softplus"]
NONE = 6
OUT = 16          # padded output width of every FFMLP
Z_MAX = 8.0       # above 8.87 the fp32 expf(10 z) of softplus overflows, kernel and reference alike
SHARE_CAP = 0.05  # largest bit-identical allowance; a case that needs more changes its inputs

# a. every <W, IN_KS, NH> instantiation (ReLU, through the module): (in_dim, hidden, num_layers)
SHAPES_RELU = ([(i, h, n) for h in (32, 64) for n in (2, 3, 4) for i in (32, 64)]
               + [(i, h, n) for (h, n) in ((64, 2), (32, 4)) for i in (16, 48)])
B_RELU, OUT_RELU = 257, 5
# b. hidden activations through the generic kernels
SHAPES_ACT = [(32, 64, 2), (48, 32, 4), (64, 64, 3)]
B_ACT = 513
# c. output activations
SHAPE_OUT, B_OUT = (32, 64, 2), 300
# d. batch edges
SHAPE_EDGE = (32, 64, 2)
B_SMALL = (1, 15, 33, 127)
ACTS_EDGE = (0, 3)
B_FWD_STRIDE = 2048 * 4 * 32 + 167   # past the forward's 2048-workgroup cap (4 waves x 32 rows each)
B_BWD_STRIDE = 256 * 4 * 32 + 39     # past the backward's 256-workgroup cap
# e. fp32 grad_weights / calc_grad_inputs = False
SHAPE_OPT, B_OPT = (32, 64, 3), 513
ACTS_OPT = (5, 0)
# g. squareplus and softplus over a wide range of pre-activations (x ~ N(0, 1), weight scale 1.5)
SHAPE_WIDE, B_WIDE = (32, 64, 2), 513
ACTS_WIDE = (4, 5)


def all_cases():
    """(in_dim, hidden, num_layers, B, act, out_act, wide) of every case the GPU
    file runs; `backward` cases are those whose gradients are compared too."""
    cs = [(s + (B_RELU, 0, NONE, False), True) for s in SHAPES_RELU]
    cs += [(s + (B_ACT, a, NONE, False), True) for a in range(1, 6) for s in SHAPES_ACT]
    cs += [(SHAPE_OUT + (B_OUT, 0, oa, False), False) for oa in range(0, 7)]
    cs += [(SHAPE_EDGE + (B, a, NONE, False), True) for a in ACTS_EDGE for B in B_SMALL]
    cs += [(SHAPE_EDGE + (B_FWD_STRIDE, a, NONE, False), False) for a in ACTS_EDGE]
    cs += [(SHAPE_EDGE + (B_BWD_STRIDE, a, NONE, False), True) for a in ACTS_EDGE]
    cs += [(SHAPE_OPT + (B_OPT, a, NONE, False), True) for a in ACTS_OPT]
    cs += [(SHAPE_WIDE + (B_WIDE, a, NONE, True), True) for a in ACTS_WIDE]
    return cs


def num_params(in_dim, hidden, nl):
    return hidden * (in_dim + hidden * (nl - 1) + OUT)


X_WIDE, S_WIDE = 1.0, 1.5


def make_inputs(in_dim, hidden, nl, B, act, out_act=NONE, out_cols=OUT, wide=False):
    """x ~ N(0, 0.5), weights U(+-sqrt(3 / hidden)) * s and an output gradient
    (zero past out_cols), all fp16. s = 1, except:
      * exponential: s = 0.5 (at s = 1 a 4-layer exponential network overflows
        fp16 in the oracle itself);
      * squareplus and softplus with 3 or 4 layers: s = 0.25. At s = 1 the fp32
        formulas alone move 3.0 % (squareplus) and 2.4 % (softplus) of the
        (64, 64, 3) grad_inputs off the float64 oracle, which needs more than
        the 5 % cap (a delta that rounds the other way moves every sum it
        enters, so the share grows with the depth of the delta chain); at
        s = 0.5 single seeds still reach 2.5 %, at s = 0.25 the cases measure
        0.4 .. 1.9 %. Their pre-activations stay below 0.8;
      * wide (case g): x ~ N(0, 1) and s = 1.5 on a 2-layer network, so that
        squareplus and softplus also see |z| up to ~5, softplus's z << 0
        (where log(exp(10 z) + 1) loses its fp32 bits) included.
    The output gradient is N(0, 1) for the ReLU networks and |N(0, 1)| for the
    others. dW is a sum over the batch of products of fp16-rounded deltas; with
    gradients of both signs the sum cancels, and the deltas that an fp32
    evaluation rounds the other way (1 .. 2 % of them behind three or four
    smooth layers) already move 8 .. 14 % of such a dW off the float64 oracle,
    more than the 0.9 contract of dW admits for any kernel. With a non-negative
    gradient the sums of the last layers cancel less and the same evaluation
    moves 2 .. 9 %."""
    rng = np.random.default_rng([in_dim, hidden, nl, B, act, out_act] + [1] * wide)
    x = (rng.standard_normal((B, in_dim)) * (X_WIDE if wide else 0.5)).astype(np.float16)
    s = S_WIDE if wide else 0.5 if act == 1 else 0.25 if (act in (4, 5) and nl >= 3) else 1.0
    w = (rng.uniform(-1, 1, num_params(in_dim, hidden, nl)) * np.sqrt(3 / hidden) * s).astype(np.float16)
    g = np.zeros((B, OUT), np.float16)
    g[:, :out_cols] = rng.standard_normal((B, out_cols)).astype(np.float16)
    if act != 0:
        g = np.abs(g)
    return x, w, g


def run_f32(x, w, g, in_dim, hidden, nl, act, out_act, backward):
    """oracle.mlp_forward / mlp_backward's formulas with every product, sum and
    activation in numpy float32 (fp16 storage between layers, like the kernel).
    Returns (out, hs, grad_inputs, grad_weights fp32); the grads are None
    without `backward`."""
    f = np.float32
    mats = oracle.mlp_layers(np.asarray(w, np.float16).astype(f), in_dim, OUT, hidden, nl)
    h, hs = np.asarray(x, np.float16), []
    for li, W in enumerate(mats):
        z = h.astype(f) @ W.T
        assert z.dtype == f
        if li < len(mats) - 1:
            h = oracle._act(act, z).astype(np.float16)
            hs.append(h)
        else:
            out = oracle._act(out_act, z).astype(np.float16)
    if not backward:
        return out, hs, None, None
    ins = [np.asarray(x, np.float16).astype(f)] + [h.astype(f) for h in hs]
    d = np.asarray(g, np.float16).astype(f)
    gws = [None] * len(mats)
    for li in range(len(mats) - 1, -1, -1):
        gws[li] = d.T @ ins[li]
        g_in = d @ mats[li]
        if li > 0:
            d = oracle._act_bwd(act, g_in, ins[li]).astype(np.float16).astype(f)
        else:
            gi = g_in.astype(np.float16)
    gw = np.concatenate([a.reshape(-1) for a in gws])
    assert gw.dtype == f
    return out, hs, gi, gw


def differing(a, b):
    """Share of fp16 values whose bits differ."""
    a, b = np.asarray(a).astype(np.float16), np.asarray(b).astype(np.float16)
    return float((a.view(np.uint16) != b.view(np.uint16)).mean())


def allowance(share):
    """Bit-identical allowance of a non-ReLU tensor: twice the share that the
    fp32 formula costs on the CPU (the doubling covers the kernel's fp32 MFMA
    accumulation order, which the numpy run does not have) plus 0.5 %."""
    return 2 * share + 0.005


DW_MIN_EQUAL = 0.9  # every dW, whatever the activation: the existing contract


class Case:
    """One case's inputs and oracle results. Read-only: the arrays are shared
    among the tests that use the case."""

    def __init__(self, in_dim, hidden, nl, B, act, out_act, backward, out_cols, wide):
        self.dims = (in_dim, hidden, nl)
        self.B, self.act, self.out_act = B, act, out_act
        self.x, self.w, self.g = make_inputs(in_dim, hidden, nl, B, act, out_act, out_cols, wide)
        self.out, self.hs = oracle.mlp_forward(self.x, self.w, in_dim, OUT, hidden, nl, act, out_act)
        self.gi = self.gw = None
        if backward:
            self.gi, self.gw = oracle.mlp_backward(self.g, self.x, self.w, in_dim, OUT, hidden, nl, act)
        # pre-activations of the oracle's own (fp16-stored) layers
        mats = oracle.mlp_layers(self.w.astype(np.float64), in_dim, OUT, hidden, nl)
        ins = [self.x] + self.hs
        zs = [i.astype(np.float64) @ W.T for i, W in zip(ins, mats)]
        self.zmax = max(float(np.abs(z).max()) for z in zs)
        self.zmin_hidden = min(float(z.min()) for z in zs[:-1])
        # what an fp32 evaluation of the same formulas costs against float64
        o32, h32, gi32, gw32 = run_f32(self.x, self.w, self.g, in_dim, hidden, nl, act, out_act, backward)
        self.f32 = {"out": o32, "gi": gi32}
        self.share = {"out": differing(o32, self.out),
                      "hs": [differing(a, b) for a, b in zip(h32, self.hs)]}
        if backward:
            self.share["gi"] = differing(gi32, self.gi)
            self.share["gw"] = differing(gw32, self.gw)
        for a in [self.x, self.w, self.g, self.out, self.gi, self.gw, o32, gi32] + self.hs:
            if a is not None:
                a.setflags(write=False)

    @property
    def relu(self):
        """ReLU hidden layers, and no or a ReLU output activation."""
        return self.act == 0 and self.out_act in (0, NONE)

    def check_ranges(self, pooled=False):
        """The conditions on the oracle alone: finite hidden values and
        outputs, |z| <= 8 for every pre-activation, every allowance within the
        5 % cap, and the fp32 formula's own dW inside the 0.9 contract (a case
        that misses one of them changes its inputs). pooled: a batch of a few
        rows, whose output and grad_inputs shares are taken over the pooled
        rows of its group (check_small)."""
        for a in [self.out] + self.hs:
            assert np.isfinite(a.astype(np.float64)).all(), (self.dims, self.act, self.out_act)
        assert self.zmax <= Z_MAX, (self.dims, self.act, self.out_act, self.zmax)
        if not self.relu and not pooled:
            for s in [self.share["out"], self.share.get("gi", 0.0)] + self.share["hs"]:
                assert allowance(s) <= SHARE_CAP, (self.dims, self.act, self.out_act, self.share)
        assert self.share.get("gw", 0.0) <= 1.0 - DW_MIN_EQUAL, (self.dims, self.act, self.share)

    def min_equal(self, what):
        """close16's bit-identical share for tensor `what`: "out", "gi", "gw" or
        ("hs", layer). dW: 0.9, the existing contract, for every activation.
        ReLU cases keep close16's 0.98; the others allow allowance() of the
        tensor's own CPU-measured share."""
        if what == "gw":
            return DW_MIN_EQUAL
        if self.relu:
            return 0.98
        s = self.share["hs"][what[1]] if isinstance(what, tuple) else self.share[what]
        assert allowance(s) <= SHARE_CAP, (what, s)
        return 1.0 - allowance(s)


@functools.lru_cache(maxsize=None)
def case(in_dim, hidden, nl, B, act=0, out_act=NONE, backward=True, out_cols=OUT, wide=False):
    return Case(in_dim, hidden, nl, B, act, out_act, backward, out_cols, wide)


def get(spec, backward):
    """The Case of an all_cases() entry (module cases use OUT_RELU live columns)."""
    in_dim, hidden, nl, B, act, out_act, wide = spec
    out_cols = OUT_RELU if (B == B_RELU and act == 0 and out_act == NONE) else OUT
    return case(in_dim, hidden, nl, B, act, out_act, backward, out_cols, wide)


# ---- batches of a few rows -----------------------------------------------------
# A share measured on n values is a count out of n: the 16 outputs of a 1-row
# batch resolve 6 %, and the CPU run of a 33-row batch can show 0 differing
# values of 528 where the rate is 1 %. So a non-ReLU group measures its rate on
# the pooled rows of its batches, rate = allowance(pooled CPU share), and each
# batch of n values may differ in n * rate values plus three standard
# deviations of a binomial count at that rate, 3 sqrt(n rate (1 - rate)).
# ReLU batches keep close16's 0.98 each.

def small_cases(act):
    return [case(*SHAPE_EDGE, B, act) for B in B_SMALL]


def pooled_rate(cases, what):
    s = differing(np.concatenate([c.f32[what] for c in cases]),
                  np.concatenate([getattr(c, what) for c in cases]))
    assert allowance(s) <= SHARE_CAP, (what, s)
    return allowance(s)


def pooled_min_equal(cases, what):
    """min_equal of the pooled rows of a group ("out" or "gi")."""
    return 0.98 if all(c.relu for c in cases) else 1.0 - pooled_rate(cases, what)


def small_min_equal(cases, c, what):
    """min_equal of batch c of the group on its own."""
    if c.relu:
        return 0.98
    rate, n = pooled_rate(cases, what), getattr(c, what).size
    return 1.0 - (rate + 3 * (rate * (1 - rate) / n) ** 0.5)


def check_small(cases):
    for c in cases:
        c.check_ranges(pooled=True)
    for what in ("out", "gi"):
        assert 1.0 - SHARE_CAP <= pooled_min_equal(cases, what) <= 1.0
