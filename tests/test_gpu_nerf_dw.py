"""GPU: the light regime of the NeRF backward through the C ABI
(ngp_nerf_backward_live_dw, ngp_nerf_dw_reduce: k_nerf_bwd<NHS, NHC, true> and the
row-order dW product of csrc/ngp_reduce.h) on all four depth pairs, against
ngp_nerf_backward_live + ngp_ffmlp_reduce and the float64 oracle, and the
fused trainer with the option dw_rows on against off.

Inputs, counts, lists and references: tests/nerf_dw_cases.py (the 161-row
cases of tests/nerf_net_cases.py inside an allocation of 300 rows); their
conditions: tests/test_nerf_dw_cases_cpu.py.
Every output starts as a NaN sentinel, every unlisted input row is NaN, and the
stash starts as NaN bytes: nothing of an unlisted row or of a stale stash may
reach an output. dW is held to the oracle by the rule tests/test_gpu_nerf_net.py
applies to ngp_nerf_backward_live (helpers.close16, 0.9 of the values
bit-identical), the sigma network's on the device's own g_h.
"""
import ctypes

import numpy as np
import pytest
import torch

import ffmlp_cases as fc
import nerf_dw_cases as dc
import nerf_net_cases as nc
import test_gpu_nerf_net as tn
from helpers import close16

pytestmark = pytest.mark.gpu

WS_FILL = 7   # the workspaces' bytes before a light launch, which must not touch them


def stash_of(cuda, rows, nl, nlc):
    _, lib, _ = tn._nat()
    n = int(lib.ngp_nerf_dw_stash_bytes(rows, nl, nlc))
    assert n == -(-rows // 32) * (48 + 128 * nl + 48 + 128 * nlc) * 64   # ngp_reduce.h's record
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=cuda)   # fp16 NaNs


def nan_dw(cuda, nl, nlc):
    return [torch.full((nc.num_params(k),), float("nan"), dtype=torch.float16, device=cuda) for k in (nl, nlc)]


def dw_backward(cuda, nets, nl, nlc, inputs, rows, n, rows_max, stash, stash_rows, fill=WS_FILL, gw=None, flag=None):
    """ngp_nerf_backward_live_dw + ngp_nerf_dw_reduce over rows[:n]: (g_h, g_enc,
    (dW sigma, dW colour), workspaces)."""
    nat, lib, P = tn._nat()
    (_, _), (im_s, im_c) = nets
    go, ci, gh, encp, genc = inputs
    gh, genc = gh.clone(), genc.clone()
    wsb = tn.workspaces(cuda, dc.B_ALLOC, nl, nlc, fill)
    rd = tn.dev(rows, cuda) if len(rows) else torch.zeros(1, dtype=torch.int32, device=cuda)
    cnt = tn.count_of(n, cuda)
    gw = gw or nan_dw(cuda, nl, nlc)
    nat.check(lib.ngp_nerf_backward_live_dw(P(go), P(ci), P(im_c), P(gh), P(encp), P(im_s), P(genc), dc.B_ALLOC, P(rd),
                                            P(cnt), 64, nl, 64, nlc, P(wsb[0]), wsb[0].numel(), P(wsb[1]),
                                            wsb[1].numel(), None, P(stash), stash_rows, rows_max, None),
              "nerf_backward_live_dw")
    nat.check(lib.ngp_nerf_dw_reduce(tn.arr(wsb), tn.u32([dc.B_ALLOC, dc.B_ALLOC]), tn.u32([32, 32]), tn.u32([64, 64]),
                                     tn.u32([nl, nlc]), tn.arr(gw), P(flag) if flag is not None else None, P(cnt),
                                     P(stash), stash_rows, rows_max, None), "nerf_dw_reduce")
    torch.cuda.synchronize()
    return gh, genc, gw, wsb


def live_backward(cuda, nets, nl, nlc, inputs, rows, n):
    """The existing entries over the same rows: ngp_nerf_backward_live (zeroed
    workspaces: ngp_ffmlp_reduce takes no live count) + ngp_ffmlp_reduce."""
    rd = tn.dev(rows, cuda) if len(rows) else torch.zeros(1, dtype=torch.int32, device=cuda)
    gh, genc, wsb = tn.one_launch_backward(cuda, nets, nl, nlc, inputs, dc.B_ALLOC, tn.count_of(n, cuda), rows=rd,
                                           fill=0)
    gw = tn.reduce_dw(cuda, wsb, dc.B_ALLOC, nl, nlc, tn.F16)
    torch.cuda.synchronize()
    return gh, genc, gw


def untouched(wsb, fill=WS_FILL):
    return all(bool((w == fill).all()) for w in wsb)


def check_dw(nl, nlc, kind, n, gh, gw, what):
    """Both dW against the oracle over the rows (the sigma network's on the
    device's g_h), by check_backward_rows' rule for fp16 weight gradients."""
    idx = dc.rows_of(kind, n)
    close16(tn.host(gw[1]), dc.color_reference(nl, nlc, kind, n)[1], f"{what} dW colour", min_equal=fc.DW_MIN_EQUAL)
    ref_s = dc.sigma_reference(nl, nlc, kind, n, tn.host(gh)[idx])[1]
    close16(tn.host(gw[0]), ref_s, f"{what} dW sigma", min_equal=fc.DW_MIN_EQUAL)


@pytest.fixture(scope="module")
def nets_of(cuda):
    made = {}

    def get(nl, nlc):
        if (nl, nlc) not in made:
            c = dc.case(nl, nlc)
            made[nl, nlc] = tn.pack_pair(cuda, c.w_sigma, c.w_color, nl, nlc)
        return made[nl, nlc]
    return get


def inputs_of(cuda, nl, nlc, rows, g=None, cin=None):
    c = dc.case(nl, nlc)
    return tn.backward_inputs(cuda, dc.padded(c.g if g is None else g), dc.padded(c.color_in if cin is None else cin),
                              dc.padded(c.g_h0), dc.padded(c.enc), np.array(rows))


@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("nl,nlc", dc.PAIRS)
def test_light_path_equals_live_backward(cuda, nets_of, nl, nlc, kind):
    """Every count up to the switch, on each kind of row list: g_h[:, 1:16] and
    g_enc bit for bit those of ngp_nerf_backward_live, the unlisted rows'
    sentinels kept, both dW within the oracle rule and bit for bit those of
    ngp_ffmlp_reduce, the workspaces untouched (the light regime ran), and with
    no row exact zeros."""
    nets = nets_of(nl, nlc)
    for n in dc.COUNTS:
        rows = dc.rows_of(kind, n)
        inputs = inputs_of(cuda, nl, nlc, rows)
        stash = stash_of(cuda, dc.STASH_ROWS, nl, nlc)
        gh, genc, gw, wsb = dw_backward(cuda, nets, nl, nlc, inputs, rows, n, dc.ROWS_MAX, stash, dc.STASH_ROWS)
        gh0, genc0, gw0 = live_backward(cuda, nets, nl, nlc, inputs, rows, n)
        what = f"{nl}/{nlc} {kind} {n}"
        assert tn.same_bits(gh, gh0) and tn.same_bits(genc, genc0), what
        unlisted = np.ones(dc.B_ALLOC, bool)
        unlisted[rows] = False
        um = tn.dev(unlisted, cuda)
        assert tn.kept(gh[um]) and tn.kept(genc[:, um]), what
        assert untouched(wsb), what
        if n == 0:
            assert all(bool((g.view(torch.int16) == 0).all()) for g in gw), what   # +0.0 everywhere
            continue
        assert tn.same_bits(gh[tn.dev(rows.astype(np.int64), cuda), 0], inputs[2][tn.dev(rows.astype(np.int64), cuda), 0])
        check_dw(nl, nlc, kind, n, gh, gw, what)
        # the product sums in the slab path's order (ngp_reduce.h): the same bits
        assert all(tn.same_bits(a, b) for a, b in zip(gw, gw0)), what


@pytest.mark.parametrize("nl,nlc", dc.PAIRS)
def test_switch_at_rows_max(cuda, nets_of, nl, nlc):
    """64 rows with dw_rows_max 64 run light; 65 rows, and any count with
    dw_rows_max 0, run the existing path: every output, dW bits included,
    equals ngp_nerf_backward_live + ngp_ffmlp_reduce, and the workspaces hold
    the slab rows."""
    nets = nets_of(nl, nlc)
    for n, rows_max, light in ((64, 64, True), (65, 64, False), (32, 0, False), (0, 0, False)):
        rows = dc.rows_of("rays", n)
        inputs = inputs_of(cuda, nl, nlc, rows)
        stash = stash_of(cuda, dc.STASH_ROWS, nl, nlc)
        gh, genc, gw, wsb = dw_backward(cuda, nets, nl, nlc, inputs, rows, n, rows_max, stash, dc.STASH_ROWS, fill=0)
        gh0, genc0, gw0 = live_backward(cuda, nets, nl, nlc, inputs, rows, n)
        assert tn.same_bits(gh, gh0) and tn.same_bits(genc, genc0), (n, rows_max)
        assert untouched(wsb, 0) == (light or n == 0), (n, rows_max)
        if not light:
            assert all(tn.same_bits(a, b) for a, b in zip(gw, gw0)), (n, rows_max)
            assert bool((stash == 0xFF).all()), (n, rows_max)   # the heavy regime stashes nothing
    # a stash shorter than dw_rows_max caps the switch at its whole chunks
    rows = dc.rows_of("rays", 33)
    inputs = inputs_of(cuda, nl, nlc, rows)
    stash = stash_of(cuda, 32 + 31, nl, nlc)
    _, _, gw, wsb = dw_backward(cuda, nets, nl, nlc, inputs, rows, 33, dc.ROWS_MAX, stash, 32 + 31)
    assert not untouched(wsb)
    check_dw(nl, nlc, "rays", 33, live_backward(cuda, nets, nl, nlc, inputs, rows, 33)[0], gw, "short stash")


@pytest.mark.parametrize("nl,nlc", dc.PAIRS)
def test_stale_stash_and_determinism(cuda, nets_of, nl, nlc):
    """96 rows, then 32 rows over the same stash and outputs: the second result
    equals a run on fresh NaN-filled buffers bit for bit (chunks past the count
    are not read). The same call twice gives the same dW bits."""
    nets = nets_of(nl, nlc)
    n0, n1 = dc.STALE
    stash = stash_of(cuda, dc.STALE_ROWS_MAX, nl, nlc)
    gw = nan_dw(cuda, nl, nlc)
    rows0, rows1 = dc.rows_of("strided", n0), dc.rows_of("strided", n1)
    in0, in1 = inputs_of(cuda, nl, nlc, rows0), inputs_of(cuda, nl, nlc, rows1)
    _, _, gw_a, wsb = dw_backward(cuda, nets, nl, nlc, in0, rows0, n0, dc.STALE_ROWS_MAX, stash, dc.STALE_ROWS_MAX,
                                  gw=gw)
    assert untouched(wsb)
    first = [g.clone() for g in gw_a]
    check_dw(nl, nlc, "strided", n0, live_backward(cuda, nets, nl, nlc, in0, rows0, n0)[0], first, "96 rows")
    gh_b, genc_b, gw_b, _ = dw_backward(cuda, nets, nl, nlc, in1, rows1, n1, dc.STALE_ROWS_MAX, stash,
                                        dc.STALE_ROWS_MAX, gw=gw)
    second = [g.clone() for g in gw_b]
    fresh = stash_of(cuda, dc.STALE_ROWS_MAX, nl, nlc)
    gh_c, genc_c, gw_c, _ = dw_backward(cuda, nets, nl, nlc, in1, rows1, n1, dc.STALE_ROWS_MAX, fresh,
                                        dc.STALE_ROWS_MAX)
    assert tn.same_bits(gh_b, gh_c) and tn.same_bits(genc_b, genc_c)
    assert all(tn.same_bits(a, b) for a, b in zip(second, gw_c))
    assert all(tn.same_bits(a, b) for a, b in zip(second, live_backward(cuda, nets, nl, nlc, in1, rows1, n1)[2]))
    assert not any(tn.same_bits(a, b) for a, b in zip(first, second))
    # determinism: the same call again, on the stash the last call left
    _, _, gw_d, _ = dw_backward(cuda, nets, nl, nlc, in1, rows1, n1, dc.STALE_ROWS_MAX, fresh, dc.STALE_ROWS_MAX)
    assert all(tn.same_bits(a, b) for a, b in zip(gw_c, gw_d))


@pytest.mark.parametrize("nl,nlc", dc.PAIRS)
def test_nonfinite_flag(cuda, nets_of, nl, nlc):
    """A row scaled so that a colour dW entry passes fp16's range sets the flag
    in the light regime; the unscaled rows leave it 0."""
    nets = nets_of(nl, nlc)
    rows, g, cin = dc.overflow_rows(nl, nlc)
    for scaled in (False, True):
        flag = torch.zeros(2, dtype=torch.int32, device=cuda)
        inputs = inputs_of(cuda, nl, nlc, rows, g if scaled else None, cin if scaled else None)
        stash = stash_of(cuda, dc.STASH_ROWS, nl, nlc)
        _, _, gw, wsb = dw_backward(cuda, nets, nl, nlc, inputs, rows, len(rows), dc.ROWS_MAX, stash, dc.STASH_ROWS,
                                    flag=flag)
        assert untouched(wsb)
        assert int(flag[0]) == int(scaled)
        assert bool(torch.isfinite(gw[1].float()).all()) == (not scaled)


def _oracle_dw(t, rows):
    """The float64 dW of both networks over the live rows of trainer t's last
    backward, from its own buffers (the sigma network on its device g_h)."""
    c = t.col_net
    s = t.sig_net
    idx = rows.long()
    g, cin = tn.host(t.g_color_out[idx]), tn.host(t.color_in[idx])
    gh = tn.host(t.g_h[idx])
    enc = nc.row_major(tn.host(t.enc_out.view(16, -1, 2)[:, idx].contiguous()))
    gw_c = nc.color_backward(g, cin, tn.host(t.w_half[2]), c.num_layers)[1]
    gw_s = nc.sigma_backward(gh, enc, tn.host(t.w_half[1]), s.num_layers)[1]
    return gw_s, gw_c


def test_trainer_dw_rows_on_against_off(cuda):
    """The fused trainer on a small scene with dw_rows on (every step light:
    the threshold is past the kernels' own cap) against off, from one seed. Step 1: the
    sample count, the live-row list, the loss and the table gradient bit for
    bit; both MLP gradients within close16's per-value tolerance of the float64
    oracle over the trainer's own live rows. (The rule's bit-identical share is
    stated for non-negative output gradients, nerf_net_cases.make_rows: a
    training step's gradients have both signs, its sums cancel, and no
    evaluation order keeps 0.9 of such a dW's bits; the per-value bound and the
    whole-tensor norm hold whatever the signs.) Then 30 steps, eager and in a
    captured multi-step graph: the same sample counts, the loss within the
    tolerance tests/test_gpu_fused.py holds the fused step to against autograd."""
    import test_gpu_fused as tf
    kw = dict(bound=2, dt_gamma=1 / 128)   # the scene of tests/test_gpu_fused.py with a few thousand live rows
    _, _, _, a = tf._setup(cuda, options=dict(dw_rows=1 << 30), **kw)
    _, _, _, b = tf._setup(cuda, options=dict(dw_rows=0), **kw)
    assert a._dw_rows and not b._dw_rows and a._live and b._live
    a.step()
    b.step()
    torch.cuda.synchronize()
    n = a.sample_count()
    assert n > 0 and n == b.sample_count()
    ta, tb = int(a._live_bufs["total"][0]), int(b._live_bufs["total"][0])
    assert 0 < ta == tb <= a._dw_cap
    # the light regime ran: no slab row was written (the workspaces start zeroed)
    assert all(int(w.count_nonzero()) == 0 for w in a.mlp_ws) and all(int(w.count_nonzero()) > 0 for w in b.mlp_ws)
    rows = a._live_bufs["rows"][:ta]
    assert torch.equal(rows, b._live_bufs["rows"][:tb])
    assert torch.equal(a.loss_ray, b.loss_ray)
    assert tn.same_bits(a.g_enc, b.g_enc) and tn.same_bits(a.g_h, b.g_h)
    assert tn.same_bits(a.grads[0], b.grads[0])
    ref = _oracle_dw(a, rows)
    for k, name in ((1, "sigma"), (2, "colour")):
        assert torch.isfinite(a.grads[k].float()).all(), name
        close16(tn.host(a.grads[k]), ref[k - 1], f"trainer dW {name}", min_equal=0.0)
        close16(tn.host(b.grads[k]), ref[k - 1], f"trainer dW {name} (off)", min_equal=0.0)
        assert tn.same_bits(a.grads[k], b.grads[k]), name   # the slab path's summation order
    assert a.last_loss == b.last_loss
    counts = {id(a): [n], id(b): [n]}
    losses = {id(a): [a.last_loss], id(b): [b.last_loss]}
    for t in (a, b):
        for _ in range(4):   # steps 2..5 eager
            t.step()
            counts[id(t)].append(t.sample_count())
            losses[id(t)].append(t.last_loss)
        t.capture(warmup=1, multi=4)   # step 6
        for _ in range(6):   # 24 steps in the graph of 4
            t.run(4)
            counts[id(t)].append(t.sample_count())
            losses[id(t)].append(t.last_loss)
        t.flush()
    torch.cuda.synchronize()
    assert counts[id(a)] == counts[id(b)]
    for x, y in zip(losses[id(a)], losses[id(b)]):
        assert np.isfinite(x) and abs(x - y) <= 1e-3 * abs(y) + 1e-7, (x, y)
