"""CPU: the conditions tests/test_gpu_nerf_dw.py rests on, checked on the
float64 oracle and its fp32 restatement without a device (tests/nerf_dw_cases.py).
"""
import numpy as np
import pytest

import ffmlp_cases as fc
import nerf_dw_cases as dc
import nerf_net_cases as nc


def test_lists_cover_the_chunk_edges():
    """Counts at every edge of the 16-row halves and 32-row chunks up to the
    switch; every list inside the allocation without a repeated row; the ray
    list not ascending; the stash large enough for the switch."""
    assert dc.COUNTS == (0, 1, 15, 16, 17, 31, 32, 33, 63, 64) and max(dc.COUNTS) == dc.ROWS_MAX
    assert dc.STASH_ROWS >= dc.ROWS_MAX and dc.STASH_ROWS % 32 == 0
    assert dc.STALE[0] <= dc.STALE_ROWS_MAX and dc.STALE[0] > dc.STALE[1] and dc.STALE[1] % 32 == 0
    for kind in dc.KINDS:
        rows = dc.row_list(kind)
        assert len(rows) == 96 and len(set(rows.tolist())) == 96
        assert rows.min() >= 0 and rows.max() < dc.B
    assert np.all(np.diff(dc.row_list("contiguous")) == 1)
    assert np.all(np.diff(dc.rows_of("strided", 64)) == 2)
    assert (np.diff(dc.row_list("rays")) < 0).any()
    # the allocation runs on three workgroups: every list up to the stale-stash test's 96 rows is
    # at most one chunk per workgroup, the light regime's condition
    assert nc.bwd_blocks(dc.B_ALLOC) == 3 and dc.B_ALLOC > dc.B
    assert max(dc.STALE) <= 32 * nc.bwd_blocks(dc.B_ALLOC)


@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("nl,nlc", dc.PAIRS)
def test_fp32_dw_meets_the_rule_on_every_list(nl, nlc, kind):
    """The dW rule of tests/test_gpu_nerf_net.py (close16 against the float64
    oracle, 0.9 of the values bit-identical) is met by the fp32 restatement on
    every row list the device runs, the switch's 65 rows and the stale-stash
    lists included: no list holds a ReLU unit at the edge of zero
    (nerf_net_cases.check_dw_rows)."""
    c = dc.case(nl, nlc)
    c.check_ranges(pooled=True)
    for n in [k for k in dc.COUNTS if k] + [dc.ROWS_MAX + 1] + list(dc.STALE):
        nc.check_dw_rows(c, dc.rows_of(kind, n))


@pytest.mark.parametrize("nl,nlc", dc.PAIRS)
def test_overflow_row_overflows_a_weight_gradient(nl, nlc):
    """The nonfinite case: the oracle's colour dW over its rows holds a value
    that fp16 cannot (past its largest; or not finite, where already a delta
    overflowed in the oracle's fp16 storage), and none without the scaled row."""
    c = dc.case(nl, nlc)
    rows, g, cin = dc.overflow_rows(nl, nlc)
    assert np.isfinite(g.astype(np.float64)).all() and np.isfinite(cin.astype(np.float64)).all()
    gw = nc.color_backward(g[rows], cin[rows], c.w_color, nlc)[1]
    with np.errstate(invalid="ignore"):
        assert not np.all(np.abs(np.asarray(gw, np.float64)) <= 65504.0 * (1 + 2.0 ** -11))
    gw0 = dc.color_reference(nl, nlc, "contiguous", 32)[1]
    assert np.abs(np.asarray(gw0, np.float64)).max() < 0.5 * 65504.0


def test_references_are_shared_and_read_only():
    nl, nlc = dc.PAIRS[0]
    a = dc.color_reference(nl, nlc, "rays", 33)
    assert a is dc.color_reference(nl, nlc, "rays", 33)
    assert dc.case(nl, nlc) is nc.case(nl, nlc, dc.B, True)
    assert not dc.case(nl, nlc).g.flags.writeable
    assert fc.DW_MIN_EQUAL == 0.9
