"""Inputs of the light-regime tests of the NeRF backward (ngp_nerf_backward_live_dw
with ngp_nerf_dw_reduce, tests/test_gpu_nerf_dw.py): the row lists, their
counts and the float64 references, on the 161-row backward cases of
tests/nerf_net_cases.py (shared with tests/test_gpu_nerf_net.py, read-only).

The light regime is switched by the live-row count, so the tests pass
dw_rows_max = 64 and walk the counts at which the chunk arithmetic changes:
no row, one row, one short of / at / past a 16-row half chunk and a 32-row
chunk, and the same around the second chunk up to the switch itself.
tests/test_nerf_dw_cases_cpu.py holds the conditions on these inputs.
"""
import functools

import numpy as np

import nerf_net_cases as nc

B = 161                    # rows of the cases: nc.B_BWD_SMALL's largest
B_ALLOC = 300              # allocated rows (the cases' rows, then rows no list names): three backward
                           # workgroups, so that up to 96 rows are one chunk per workgroup (the light
                           # regime's condition, ffmlp.hip dw_rows_limit)
ROWS_MAX = 64              # dw_rows_max of the tests
STASH_ROWS = 96            # the stash's capacity in rows (>= ROWS_MAX)
COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64)
KINDS = ("contiguous", "strided", "rays")
PAIRS = nc.BWD_PAIRS
# rays of the batch as the marcher lays them out: runs of consecutive rows
RAY_RUNS = ((0, 21), (21, 47), (47, 80), (80, 131), (131, 161))
RAY_ORDER = (3, 0, 4, 2, 1)   # the order the composite lists them in (not ascending)
STALE = (96, 32)           # a long list, then a short one over the same stash
STALE_ROWS_MAX = 128


def case(nl, nlc):
    return nc.case(nl, nlc, B, True)


def padded(a):
    """The case's rows, then zeros up to the allocation (no list names those rows)."""
    a = np.asarray(a)
    return np.concatenate([a, np.zeros((B_ALLOC - len(a),) + a.shape[1:], a.dtype)])


@functools.lru_cache(maxsize=None)
def row_list(kind):
    """The longest list of a kind (96 rows, every row at most once); a count n
    takes its first n rows."""
    if kind == "contiguous":
        rows = np.arange(40, 136)
    elif kind == "strided":
        rows = np.concatenate([np.arange(1, B, 2), np.arange(0, 32, 2)])
    else:
        rows = np.concatenate([np.arange(*RAY_RUNS[k]) for k in RAY_ORDER])[:96]
    rows = rows.astype(np.int32)
    rows.setflags(write=False)
    return rows


def rows_of(kind, n):
    return row_list(kind)[:n]


@functools.lru_cache(maxsize=None)
def color_reference(nl, nlc, kind, n):
    """(input gradient [n, 32], dW float64) of the colour network over the rows."""
    c, idx = case(nl, nlc), rows_of(kind, n)
    return nc.color_backward(c.g[idx], c.color_in[idx], c.w_color, nlc)


def sigma_reference(nl, nlc, kind, n, g_h):
    """(g_enc [n, 32], dW float64) of the sigma network over the rows, on the
    output gradient g_h [n, 16] the device's colour pass produced."""
    c, idx = case(nl, nlc), rows_of(kind, n)
    return nc.sigma_backward(g_h, c.enc[idx], c.w_sigma, nl)


def overflow_rows(nl, nlc):
    """(rows, g, color_in) of the nonfinite-flag case: 32 contiguous rows whose
    first row is scaled, its colour output gradient to 60000 in every column
    and its colour input by 16. The cases' post-activations stay below 0.5, so
    the gradient alone (at most 65504 in fp16) overflows no dW entry; with the
    input scaled too the last layer's dW (60000 times a post-activation above
    1.1) passes fp16's 65504."""
    c, rows = case(nl, nlc), rows_of("contiguous", 32)
    g, cin = np.array(c.g), np.array(c.color_in)
    g[rows[0]] = np.float16(60000.0)
    cin[rows[0]] = (cin[rows[0]].astype(np.float32) * 16).astype(np.float16)
    return rows, g, cin
