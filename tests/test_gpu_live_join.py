"""GPU: the live-row list joined inside the NeRF backward, through the C ABI
(ngp_nerf_composite_loss_lists + ngp_nerf_backward_join_dw: k_nerf_bwd<NHS, NHC,
true, true>) against the two-launch composite with the one-launch backward on
its list (ngp_nerf_composite_loss_live: the composite and k_live_compact, then
ngp_nerf_backward_live_dw), on the same inputs and all four depth pairs: the
list, its total, g_h, g_enc, the workspaces and the weight gradients of
ngp_nerf_dw_reduce (by the stash route and by the slab route) bit for bit.
And the fused trainer with the option join_in_bwd on against off.

Inputs, planned lists and the restated arithmetic: tests/live_join_cases.py;
the cases' conditions: tests/test_live_join_cases_cpu.py. Every output starts
as a NaN sentinel, the backward's inputs are NaN on every unlisted row, the
stash starts as NaN bytes, and live_rows starts as -1: an entry past the total
must keep it.
"""
import numpy as np
import pytest
import torch

import live_join_cases as jc
import nerf_dw_cases as dc
import test_gpu_nerf_dw as td
import test_gpu_nerf_net as tn

pytestmark = pytest.mark.gpu

ERR_ARG = -1
WS_FILL = 0


@pytest.fixture(scope="module")
def nets_of(cuda):
    made = {}

    def get(nl, nlc):
        if (nl, nlc) not in made:
            c = dc.case(nl, nlc)
            made[nl, nlc] = tn.pack_pair(cuda, c.w_sigma, c.w_color, nl, nlc)
        return made[nl, nlc]
    return get


def composite(cuda, d, join):
    """The composite over a case on fresh buffers: its two-launch form with the
    finished list, or the lists form. (g_col, g_h, ray_rows, cnt, rows, total)."""
    nat, lib, P = tn._nat()
    N, M = d["N"], d["M"]
    t = lambda a: tn.dev(a, cuda)  # noqa: E731
    ins = dict(sigma=t(d["sigma"]), col=t(d["col"]), h=t(d["h"]), deltas=t(d["deltas"]), rays=t(d["rays"]),
               gt=t(d["gt"]), bg=t(d["bg"]))
    half = lambda: torch.full((M, 16), 7.0, dtype=torch.float16, device=cuda)  # noqa: E731
    i32 = torch.int32
    o = dict(g_col=half(), g_h=half(), loss=torch.full((N,), -1.0, device=cuda),
             ray_rows=torch.zeros(M, dtype=i32, device=cuda), cnt=torch.full((N,), -1, dtype=i32, device=cuda),
             rows=torch.full((M,), -1, dtype=i32, device=cuda), total=torch.full((4,), -1, dtype=i32, device=cuda))
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
    nat.check(lib.ngp_fused_state_init(P(state), jc.SCALE, None), "fused_state_init")
    args = (P(ins["sigma"]), P(ins["col"]), P(ins["h"]), P(ins["deltas"]), P(ins["rays"]), M, N, jc.T_THRESH, 1.0,
            P(ins["gt"]), 4, P(ins["bg"]), P(state), P(o["g_col"]), P(o["g_h"]), None, None, P(o["loss"]),
            P(o["ray_rows"]), P(o["cnt"]))
    if join:
        nat.check(lib.ngp_nerf_composite_loss_lists(*args, None), "composite_loss_lists")
    else:
        nat.check(lib.ngp_nerf_composite_loss_live(*args, P(o["rows"]), P(o["total"]), None), "composite_loss_live")
    torch.cuda.synchronize()
    return o, ins["rays"]


def reduce_dw(cuda, nl, nlc, wsb, M, total, stash, stash_rows, rows_max):
    nat, lib, P = tn._nat()
    gw = td.nan_dw(cuda, nl, nlc)
    nat.check(lib.ngp_nerf_dw_reduce(tn.arr(wsb), tn.u32([M, M]), tn.u32([32, 32]), tn.u32([64, 64]),
                                     tn.u32([nl, nlc]), tn.arr(gw), None, P(total), P(stash), stash_rows, rows_max,
                                     None), "nerf_dw_reduce")
    torch.cuda.synchronize()
    return gw


def run_case(cuda, nets, nl, nlc, name):
    nat, lib, P = tn._nat()
    c, d = jc.case(name), jc.build(name)
    N, M, total = c.N, c.M, len(d["rows"])
    (_, _), (im_s, im_c) = nets
    # the composite, both forms: the same gradients and per-ray lists; the planned counts and list
    ref, rays = composite(cuda, d, False)
    new, _ = composite(cuda, d, True)
    assert np.array_equal(tn.host(ref["cnt"]), d["counts"]), name
    assert int(ref["total"][0]) == total, name
    assert np.array_equal(tn.host(ref["rows"])[:total], d["rows"]) and bool((ref["rows"][total:] == -1).all()), name
    for k in ("g_col", "g_h"):
        assert tn.same_bits(ref[k], new[k]), (name, k)
    for k in ("ray_rows", "cnt", "loss"):
        assert torch.equal(ref[k], new[k]), (name, k)
    assert bool((new["rows"] == -1).all()) and bool((new["total"] == -1).all()), name   # the lists form stops there
    # the backward's inputs: the composite's gradients on the live rows, NaN elsewhere
    inputs = tn.backward_inputs(cuda, tn.host(ref["g_col"]), np.array(d["cin"]), tn.host(ref["g_h"])[:, 0],
                                np.array(d["enc"]), np.array(d["rows"], np.int64))
    go, ci, gh0, encp, genc0 = inputs
    out = {}
    for form in ("list", "join"):
        gh, genc = gh0.clone(), genc0.clone()
        wsb = tn.workspaces(cuda, M, nl, nlc, WS_FILL)
        stash = td.stash_of(cuda, c.stash_rows, nl, nlc)
        if form == "list":
            rows, tot = ref["rows"], ref["total"]
            nat.check(lib.ngp_nerf_backward_live_dw(P(go), P(ci), P(im_c), P(gh), P(encp), P(im_s), P(genc), M,
                                                    P(rows), P(tot), 64, nl, 64, nlc, P(wsb[0]), wsb[0].numel(),
                                                    P(wsb[1]), wsb[1].numel(), None, P(stash), c.stash_rows,
                                                    c.rows_max, None), "nerf_backward_live_dw")
        else:
            rows, tot = new["rows"], new["total"]
            nat.check(lib.ngp_nerf_backward_join_dw(P(go), P(ci), P(im_c), P(gh), P(encp), P(im_s), P(genc), M,
                                                    P(rays), N, P(new["cnt"]), P(new["ray_rows"]), P(rows), P(tot),
                                                    64, nl, 64, nlc, P(wsb[0]), wsb[0].numel(), P(wsb[1]),
                                                    wsb[1].numel(), None, P(stash), c.stash_rows, c.rows_max, None),
                      "nerf_backward_join_dw")
        torch.cuda.synchronize()
        gw = reduce_dw(cuda, nl, nlc, wsb, M, tot, stash, c.stash_rows, c.rows_max)
        out[form] = dict(gh=gh, genc=genc, wsb=wsb, stash=stash, gw=gw, rows=rows, total=tot)
    a, b = out["list"], out["join"]
    what = f"{nl}/{nlc} {name}"
    assert int(b["total"][0]) == total, what
    assert torch.equal(b["rows"][:total], a["rows"][:total]), what
    assert bool((b["rows"][total:] == -1).all()), what
    assert tn.same_bits(a["gh"], b["gh"]) and tn.same_bits(a["genc"], b["genc"]), what
    assert all(torch.equal(x, y) for x, y in zip(a["wsb"], b["wsb"])), what
    assert torch.equal(a["stash"], b["stash"]), what
    assert all(tn.same_bits(x, y) for x, y in zip(a["gw"], b["gw"])), what
    # the regime the case is meant for ran: the stash route leaves the workspaces alone
    light = total <= jc.light_limit(M, c.rows_max, c.stash_rows) and jc.light_limit(M, c.rows_max, c.stash_rows) > 0
    assert td.untouched(b["wsb"], WS_FILL) == (light or total == 0), what
    # the unlisted rows keep their sentinels, the listed ones are written
    unlisted = np.ones(M, bool)
    unlisted[d["rows"]] = False
    um = tn.dev(unlisted, cuda)
    assert tn.kept(b["gh"][um]) and tn.kept(b["genc"][:, um]), what
    if total:
        lm = tn.dev(~unlisted, cuda)
        assert not bool(torch.isnan(b["genc"][:, lm].float()).any()), what
        assert not bool(torch.isnan(b["gh"][lm].float()).any()), what


SMALL = [c.name for c in jc.cases() if c.N < jc.CAP]
LARGE = [c.name for c in jc.cases() if c.N == jc.CAP]


@pytest.mark.parametrize("nl,nlc", dc.PAIRS)
def test_join_equals_compact_then_backward_small(cuda, nets_of, nl, nlc):
    """Every case of under 4096 rays (ray counts around a thread's group and a
    wave, the count patterns, the switch at dw_rows, 1 to 4 chunks on a
    workgroup) on each depth pair."""
    for name in SMALL:
        run_case(cuda, nets_of(nl, nlc), nl, nlc, name)


@pytest.mark.parametrize("name", LARGE)
@pytest.mark.parametrize("nl,nlc", dc.PAIRS)
def test_join_equals_compact_then_backward_full_pass(cuda, nets_of, nl, nlc, name):
    """4096 rays, the most one pass holds: the bench's shape on the stash route,
    a small allocation on the slab route, and five chunks on a workgroup."""
    run_case(cuda, nets_of(nl, nlc), nl, nlc, name)


def test_refusals(cuda, nets_of):
    """One ray past the pass (4097), and an allocation of more than 32 chunks
    per workgroup, are refused with NGP_ERR_ARG and launch nothing; a
    misaligned live_cnt too."""
    nat, lib, P = tn._nat()
    assert int(lib.ngp_nerf_backward_join_max_rays()) == jc.CAP
    (_, _), (im_s, im_c) = nets_of(2, 2)
    i32 = torch.int32

    def call(N, M, cnt_offset=0):
        half = lambda w: torch.zeros((M, w), dtype=torch.float16, device=cuda)  # noqa: E731
        go, ci, gh, genc, enc = half(16), half(32), tn.sent16((M, 16), cuda), tn.sent16((16, M, 2), cuda), half(32)
        rays = torch.zeros((N, 3), dtype=i32, device=cuda)
        cnt = torch.zeros(N + 4, dtype=i32, device=cuda)[cnt_offset:]
        rr = torch.zeros(M, dtype=i32, device=cuda)
        rows, tot = torch.full((M,), -1, dtype=i32, device=cuda), torch.full((4,), -1, dtype=i32, device=cuda)
        wsb = tn.workspaces(cuda, M, 2, 2, 0)
        stash = td.stash_of(cuda, 96, 2, 2)
        rc = lib.ngp_nerf_backward_join_dw(P(go), P(ci), P(im_c), P(gh), P(enc), P(im_s), P(genc), M, P(rays), N,
                                           P(cnt), P(rr), P(rows), P(tot), 64, 2, 64, 2, P(wsb[0]), wsb[0].numel(),
                                           P(wsb[1]), wsb[1].numel(), None, P(stash), 96, 64, None)
        torch.cuda.synchronize()
        return rc, tot, rows, gh
    rc, tot, rows, gh = call(jc.CAP + 1, 64)
    assert rc == ERR_ARG and bool((tot == -1).all()) and bool((rows == -1).all()) and tn.kept(gh)
    rc, tot, _, _ = call(64, 32 * 32 * 256 + 1)
    assert rc == ERR_ARG and bool((tot == -1).all())
    rc, tot, _, _ = call(64, 64, cnt_offset=1)
    assert rc == ERR_ARG and bool((tot == -1).all())
    # the largest shapes are taken: no live row, total 0
    rc, tot, _, _ = call(jc.CAP, 64)
    assert rc == 0 and int(tot[0]) == 0


def test_trainer_join_in_bwd_on_against_off(cuda):
    """The fused trainer from one seed with join_in_bwd on against off: 13
    steps, eager, then captured and replayed. The per-step sample and live
    counts, the live-row list, the loss, the gradients and the parameters are
    bit-identical, and the per-launch timing keeps its launch names."""
    import test_gpu_fused as tf
    kw = dict(bound=2, dt_gamma=1 / 128)   # the scene of tests/test_gpu_fused.py with a few thousand live rows
    _, _, _, a = tf._setup(cuda, options=dict(join_in_bwd=True), **kw)
    _, _, _, b = tf._setup(cuda, options=dict(join_in_bwd=False), **kw)
    assert a._join and not b._join and a._dw_rows and b._dw_rows
    seen = {id(a): [], id(b): []}

    def note(t):
        torch.cuda.synchronize()
        seen[id(t)].append((t.sample_count(), int(t._live_bufs["total"][0]), t.last_loss))

    for t in (a, b):
        for _ in range(5):   # steps 1..5 eager
            t.step()
            note(t)
    ta = int(a._live_bufs["total"][0])
    assert ta > 0 and torch.equal(a._live_bufs["rows"][:ta], b._live_bufs["rows"][:ta])
    assert tn.same_bits(a.g_enc, b.g_enc) and tn.same_bits(a.g_h, b.g_h)
    for t in (a, b):
        t.capture(warmup=1, multi=1)   # step 6
        note(t)
        for _ in range(7):   # steps 7..13 replayed
            t.step()
            note(t)
        t.flush()
    torch.cuda.synchronize()
    assert len(seen[id(a)]) == 13 and seen[id(a)] == seen[id(b)]
    assert all(n > 0 and k > 0 and np.isfinite(x) for n, k, x in seen[id(a)])
    for ga, gb in zip(a.grads, b.grads):
        assert tn.same_bits(ga, gb)
    for pa, pb in zip(a.params, b.params):
        assert tn.same_bits(pa, pb)
    # the launch names the bench indexes are the same with one launch less
    names = [sorted(t.timed_body_steps(1)[0]) for t in (a, b)]
    assert names[0] == names[1] and "composite_loss" in names[0] and "ffmlp_backward" in names[0]
