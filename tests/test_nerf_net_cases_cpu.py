"""The two-network NeRF cases (tests/nerf_net_cases.py) without a GPU: the
chained reference against torch float64 autograd, the conditions every case has
to meet before the device is touched, and the coverage the backward's batch
list is chosen for (restated from k_nerf_bwd's chunk arithmetic, so a change of
kMaxBwdBlocks or of the chunk size fails here instead of silently losing it).
"""
import numpy as np
import pytest
import torch

import ffmlp_cases as fc
import nerf_net_cases as nc
from oracle.torch_nerf import _TruncExp, sh_encode4


def torch_mlp(x, w, nl):
    """A bias-free ReLU MLP 32 -> 64 (x nl) -> 16 on FFMLP's flat weight vector:
    row-major [out, in] matrices back to back."""
    shapes = [(nc.HID, nc.IN)] + [(nc.HID, nc.HID)] * (nl - 1) + [(nc.OUT, nc.HID)]
    h, off = x, 0
    for li, (o, i) in enumerate(shapes):
        h = h @ w[off:off + o * i].view(o, i).T
        off += o * i
        if li < len(shapes) - 1:
            h = torch.relu(h)
    assert off == w.numel()
    return h


@pytest.mark.parametrize("nl,nlc", nc.FWD_PAIRS)
def test_chain_matches_torch_autograd(nl, nlc):
    """network_ff.py's forward (sigma network, trunc_exp of column 0, SH of the
    direction, cat with the geo features and a zero pad, colour network) in
    torch float64 with autograd, against nc.chain(fp16=False): the forward, the
    input gradient and both dW. The SH values differ by their float32
    evaluation in the oracle (1e-6 relative)."""
    B = 37
    ws, wc = nc.make_weights(nl, nlc)
    enc, dirs, g, g_h0 = nc.make_rows(nl, nlc, B)
    scale = 0.5
    ref = nc.chain(enc, dirs, g, g_h0, ws, wc, nl, nlc, scale, fp16=False)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())  # noqa: E731
    x, w1, w2 = t(enc).requires_grad_(True), t(ws).requires_grad_(True), t(wc).requires_grad_(True)
    h = torch_mlp(x, w1, nl)
    sigma = scale * _TruncExp.apply(h[:, 0])
    cin = torch.cat([sh_encode4(t(dirs)), h[:, 1:], torch.zeros(B, 1, dtype=torch.float64)], -1)
    cout = torch_mlp(cin, w2, nlc)
    # g_h0 is the gradient that reaches h[:, 0] (the composite kernel's output)
    ((cout * t(g)).sum() + (h[:, 0] * t(g_h0)).sum()).backward()
    close = lambda a, b, tol=1e-5: np.testing.assert_allclose(a.detach().numpy(), b, rtol=tol, atol=tol)  # noqa: E731
    close(h, ref["h"], 1e-12)
    close(sigma, ref["sigma"], 1e-6)
    close(cin, ref["color_in"])
    close(cout, ref["color_out"])
    close(x.grad, ref["g_enc"])
    close(w1.grad, ref["gw_s"], 1e-4)
    close(w2.grad, ref["gw_c"], 1e-4)
    assert ref["color_in"].shape == (B, 32) and (ref["color_in"][:, 31] == 0).all()
    assert np.array_equal(ref["g_h"][:, 0], g_h0.astype(np.float64))


@pytest.mark.parametrize("nl,nlc", nc.BWD_PAIRS)
def test_case_equals_chain(nl, nlc):
    """Case's fields are the fp16-storage chain, bit for bit, and the layouts
    are inverses of each other."""
    c = nc.case(nl, nlc, 65, True)
    ref = nc.chain(c.enc, c.dirs, c.g, c.g_h0, c.w_sigma, c.w_color, nl, nlc)
    for k in ("h", "color_in", "color_out", "gi_c", "g_h", "g_enc"):
        assert np.array_equal(getattr(c, k).view(np.uint16), ref[k].view(np.uint16)), k
    assert np.array_equal(c.gw_c, ref["gw_c"]) and np.array_equal(c.gw_s, ref["gw_s"])
    p = nc.pair_major(c.enc)
    assert p.shape == (16, 65, 2) and p[3, 7, 1] == c.enc[7, 7] and np.array_equal(nc.row_major(p), c.enc)


@pytest.mark.parametrize("spec", nc.all_cases(), ids=lambda s: "-".join(map(str, s)))
def test_case_ranges_and_share_cap(spec):
    """Finite fp16 values and pre-activations, |z| <= 8, and every share of the
    fp32 restatement within the 5 % cap (small batches: over their pool)."""
    nl, nlc, B, backward = spec
    nc.case(nl, nlc, B, backward).check_ranges(pooled=nc.is_small(B))


@pytest.mark.parametrize("nl,nlc", nc.FWD_PAIRS)
def test_small_batch_pools(nl, nlc):
    """The pooled shares stay under the cap, and every batch of a few rows meets
    the bound its pool gives it in the fp32 restatement (a 1-row batch: bit for
    bit), so that bound is one a kernel can be held to on these rows."""
    pools = [nc.forward_pool(nl, nlc)] + ([nc.backward_pool(nl, nlc)] if (nl, nlc) in nc.BWD_PAIRS else [])
    for pool in pools:
        pool.check_ranges()
        for c in pool.cases:
            for k in pool.share:
                src = pool if nc.is_small(c.B) else c
                nc.check_few_rows(c.f32[k], c.ref[k], src.min_equal(k), (c.B, k))


def test_share_table():
    """The figures of test_gpu_nerf_net.py's docstring table (largest share per
    depth pair over its cases, in %) stay below what the table states."""
    worst = {}
    for nl, nlc, B, backward in nc.all_cases():
        c = nc.case(nl, nlc, B, backward)
        small = nc.is_small(B)
        pool = (nc.backward_pool if backward else nc.forward_pool)(nl, nlc) if small else None
        for k, s in c.share.items():
            s = s if k in ("gw_c", "gw_s") or not small else pool.share[k]
            worst[k] = max(worst.get(k, 0.0), s)
    assert worst["h"] <= 0.008 and worst["color_out"] <= 0.014, worst
    assert worst["g_geo"] <= 0.008 and worst["g_enc"] <= 0.006, worst
    assert worst["gw_c"] <= 0.052 and worst["gw_s"] <= 0.029, worst


def test_edge_rows_are_exact():
    """b. the crafted h values are exactly representable, the crafted sigma
    network reproduces them bit for bit in the float64 oracle and in the fp32
    restatement, every SH value of the edge directions is finite, and sigma
    reaches 0, a subnormal-free small value and infinity."""
    h, dirs, n0 = nc.edge_h()
    assert np.array_equal(h[:n0, 0].astype(np.float64), np.array(nc.H0_EDGE))
    for v in nc.GEO_EDGE:
        assert float(np.float16(v)) == v
    assert (h.astype(np.float64) == np.float16(2.0 ** -24)).any() and np.isfinite(h.astype(np.float64)).all()
    for nl in (2, 3):
        enc, w = nc.crafted_sigma_net(h, nl)
        assert (enc >= 0).all()
        assert np.array_equal(nc.sigma_net(enc, w, nl).view(np.uint16), h.view(np.uint16))
        h32 = fc.run_f32(enc, w, np.zeros((len(h), 16), np.float16), 32, 64, nl, 0, fc.NONE, False)[0]
        assert np.array_equal(h32.view(np.uint16), h.view(np.uint16))
    cin = nc.color_in_of(h, dirs)
    assert np.isfinite(cin.astype(np.float64)).all()
    d = nc.edge_dirs()
    norms = np.linalg.norm(d.astype(np.float64), axis=-1)
    assert np.isclose(norms[:3], [0.5, 2.0, 0.0]).all() and len(d) == 10
    assert (np.abs(d[9]) > 0).all() and np.abs(d[9]).min() < np.finfo(np.float32).tiny   # a denormal component
    s = nc.sigma_of(h[:n0, 0], 1.0)
    assert s[0] == 0.0 and np.isinf(s[-1]) and np.isfinite(s[:-1]).all() and s[-2] > 1e38
    # the moderate rows keep the colour network finite
    wc = nc.make_weights(*nc.PAIR_EDGE)[1]
    assert np.isfinite(nc.color_net(cin[:n0], wc, nc.PAIR_EDGE[1]).astype(np.float64)).all()


def test_backward_batches_reach_every_chunk_split():
    """c, d. k_nerf_bwd deals a workgroup's n chunks to 4 wave slots; a last
    round of r = n mod 4 = 1 or 2 chunks is split into 2 r halves, and with
    n = 1 or 3 the colour pass's idle waves copy the sigma image. The launch
    list reaches every n mod 4, both idle-copy cases, 2 and 4 halves, a
    workgroup without chunks, and n >= 5 under the 256-workgroup cap."""
    assert nc.bwd_blocks(fc.B_BWD_STRIDE) == nc.MAX_BWD_BLOCKS == 256
    assert fc.B_BWD_STRIDE > nc.MAX_BWD_BLOCKS * nc.BWD_WAVES * nc.CHUNK
    seen_mod, seen_halves, seen_idle, seen_n = set(), set(), set(), set()
    blocks, counts = set(), set()
    for B, rows in nc.bwd_launches():
        G, plan = nc.bwd_plan(B, rows)
        blocks.add(G)
        counts.add(-(-rows // nc.CHUNK))
        for n, r, nf, halves, idle in plan:
            seen_n.add(n)
            if n:
                seen_mod.add(r)
                seen_halves.add(halves)
                if idle:
                    seen_idle.add(n)
            assert nf + (halves + 1) // 2 == n and halves in (0, 2, 4)
    assert seen_mod == {0, 1, 2, 3}
    assert seen_halves == {0, 2, 4}
    assert seen_idle == {1, 3}
    assert {0, 1, 2, 3, 4, 5} <= seen_n
    assert len(blocks) >= 3 and len(counts) >= 8   # both the grid and the chunk count vary
    # the small allocations alone: one or two workgroups with 1, 2, 3, 4, 3 + 2 and 3 + 3 chunks
    small = [tuple(p[0] for p in nc.bwd_plan(B, B)[1]) for B in nc.B_BWD_SMALL]
    assert small == [(1,), (1,), (2,), (3,), (4,), (3, 2), (3, 3)]
    # the counts inside the large allocation
    large = {c: sorted({p[0] for p in nc.bwd_plan(fc.B_BWD_STRIDE, c)[1]}) for c in nc.BWD_COUNTS}
    assert list(large.values()) == [[1, 2], [2, 3], [3], [4, 5], [0, 1], [0]]


def test_live_lists():
    """d. ascending rows inside the batch, a length that ends mid-chunk, and
    live-row launches whose last workgroups write no slab row."""
    B = fc.B_BWD_STRIDE
    ls = nc.live_lists()
    assert set(ls) == {"empty", "one", "all", "third", "mid_chunk"}
    for rows in ls.values():
        assert rows.dtype == np.int32 and (np.diff(rows) > 0).all() and ((rows >= 0) & (rows < B)).all()
    assert len(ls["all"]) == B and len(ls["mid_chunk"]) % nc.CHUNK not in (0, 16)
    assert np.array_equal(ls["third"], np.arange(0, B, 3))
    G = nc.bwd_blocks(B)
    assert nc.live_slab_rows(0, G) == 0 and nc.live_slab_rows(1, G) == 64 == nc.live_slab_rows(len(ls["mid_chunk"]), G)
    assert nc.live_slab_rows(len(ls["third"]), G) == G == nc.live_slab_rows(B, G)


@pytest.mark.parametrize("nl,nlc", nc.BWD_PAIRS)
def test_few_row_backwards_meet_the_dw_check_in_fp32(nl, nlc):
    """c, d. Over a few rows one ReLU unit at the edge of zero moves dW past its
    tolerance in any evaluation; the row sets hold none (nc.check_dw_rows)."""
    c = nc.case(nl, nlc, fc.B_BWD_STRIDE, True)
    for idx in nc.small_row_sets().values():
        nc.check_dw_rows(c, idx)
        nc.check_few_backward_rows(c, idx)
