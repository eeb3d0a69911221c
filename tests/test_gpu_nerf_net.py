"""The two-network NeRF kernels of csrc/ffmlp.hip at every depth against the
float64 oracle with fp16 storage, through the C ABI (_ngp_native):
ngp_nerf_forward (k_nerf_fwd<64, NHS, NHC>), ngp_nerf_backward and
ngp_nerf_backward_live (k_nerf_bwd<NHS, NHC>), ngp_nerf_sigma_forward
(k_mlp_fwd with EpiNerfSigma), ngp_nerf_density_forward and _rows
(k_density_fwd<W, NH>, k_mlp_fwd with EpiDensity), and the glue kernels of
csrc/nerf_fused.hip they are compared with.

Cases (tests/nerf_net_cases.py holds their inputs, references and CPU bounds;
tests/test_nerf_net_cases_cpu.py checks those without a device):
  a. the one-launch forward on all 6 depth pairs (sigma layers 2..3 x colour
     layers 2..4): B in {1, 15, 33, 127, 257}, a count that ends mid-chunk,
     counts 0 and -3, density_scale in {1, 0.5, 0}, and on one pair a batch
     past the 2048-workgroup cap (the grid-stride loop and its prefetch);
  b. epilogue edges: log densities from -65504 to 89 (no clamp in the forward,
     infinity included), geo features at +-65504 and the smallest subnormal,
     directions of norm 0.5 and 2, the zero vector, the axes and a denormal
     component, through ngp_nerf_glue_forward and through the one-launch
     forward (a sigma network crafted to give these h exactly);
     ngp_nerf_glue_backward at its batch edges;
  c. the one-launch backward on all 4 depth pairs: allocations of 1..161 rows
     (one or two workgroups with 1, 2, 3, 4, 3+2 and 3+3 chunks) and counts
     inside 32 807 allocated rows that leave the 256 workgroups 0..5 chunks,
     dW in fp16 and fp32;
  d. the live-row backward on all 4 depth pairs: an empty list, one row, every
     row, every third row, a list that ends mid-chunk;
  e. ngp_nerf_sigma_forward on the 16 shapes of ffmlp_cases.SHAPES_RELU,
     row-major and pair-major, with and without a packed image, and the shapes
     it rejects;
  f. the density forward: per row on the 6 k_density_fwd shapes, scattered with
     an image on those and without one on SHAPES_RELU, and once past the grid
     cap;
  g. FusedTrainer and FusedRenderer on NeRFNetwork(num_layers=3,
     num_layers_color=2) and (2, 4): which launches the gates choose, and the
     one-launch paths against the split ones.

Every device stage is compared against the oracle on that stage's own device
inputs (the colour network on the device's color_in, the sigma backward on the
device's g_h), with helpers.close16's tolerance: 2 fp16 ulps plus 1e-3 of the
largest magnitude; input gradients add oracle.mlp_backward_error_bound as
tests/test_gpu_e2e_oracle.py does. sigma is held to rtol 1e-6 of
float32(density_scale * exp(float64(h0))) on the device's own h0, color_in to
0.999 bit-identical (its geo columns: all), dW to 0.9. The bit-identical share
of the other tensors is measured on the CPU, never from the device: the fp32
restatement (ffmlp_cases.run_f32) of each stage against the oracle on the same
stage input; every batch, count and row list is held to min(0.98, 1 - (2 share
+ 0.5 %)), and the CPU file asserts the 5 % cap. A batch below 257 rows takes
the share of its group's pooled rows (16 values resolve 6 %) and is still held
to the rule on its own; the few-row inputs are draws on which the fp32
restatement itself meets it (nerf_net_cases.ROW_SALT, chosen on the CPU). Largest measured share per depth pair over its cases
(batches of a few rows pooled), in % of the fp16 values:

    sigma / colour layers     h  color_out  g_h[:, 1:16]  g_enc  dW colour  dW sigma
    2 / 2                  0.46       0.49          0.30   0.28       0.24      0.45
    2 / 3                  0.41       0.65          0.70   0.31       2.50      0.46
    2 / 4                  0.71       1.31             -      -          -         -
    3 / 2                  0.61       0.63          0.40   0.44       0.28      1.61
    3 / 3                  0.51       0.77          0.48   0.55       5.10      2.80
    3 / 4                  0.75       0.88             -      -          -         -

The dW columns have no allowance: they show that the fp32 formula itself stays
inside the 0.9 contract. The output gradients are |N(0, 1)| for that reason
(nerf_net_cases.make_rows: with both signs the same columns read 14 .. 25 %
over 32 807 rows).

Every output starts as a NaN sentinel and every input row at or past the count
is NaN: a row the kernels must not write keeps its bits, and nothing of a
masked row reaches a live row or a dW.
"""
import ctypes

import numpy as np
import pytest
import torch

import ffmlp_cases as fc
import nerf_net_cases as nc
from helpers import close16

pytestmark = pytest.mark.gpu

H_SENT, F_SENT = 0x7E2A, 0x7FC00ABC   # NaN bit patterns of the fp16 / fp32 outputs
F16, F32 = 1, 0                        # NGP_DTYPE_F16 / NGP_DTYPE_F32
GEO, DEFER, PAIR = 2, 1, 4             # NGP_FFMLP_NERF_GEO / _DEFER_REDUCE / _PAIR_MAJOR
ERR_UNSUPPORTED = -3


def _nat():
    import _ngp_native as nat
    return nat, nat.lib(), nat.ptr


def dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)  # a copy: the cases' arrays are read-only


def sent16(shape, cuda):
    return torch.full(shape, H_SENT, dtype=torch.int16, device=cuda).view(torch.float16)


def sent32(shape, cuda):
    return torch.full(shape, F_SENT, dtype=torch.int32, device=cuda).view(torch.float32)


def kept(t):
    """Every value still holds its sentinel bits."""
    if t.dtype == torch.float16:
        return bool((t.view(torch.int16) == H_SENT).all())
    return bool((t.view(torch.int32) == F_SENT).all())


def same_bits(a, b):
    v = torch.int16 if a.dtype == torch.float16 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def host(t):
    return t.cpu().numpy()


def nan_from(a, n):
    """A copy of `a` whose rows at or past n are NaN."""
    a = np.array(a)
    a[n:] = np.nan
    return a


def count_of(count, cuda):
    return None if count is None else torch.tensor([count, 0], dtype=torch.int32, device=cuda)


def clip(B, count):
    return B if count is None else max(0, min(B, count))


def arr(ts):
    _, _, P = _nat()
    return (ctypes.c_void_p * len(ts))(*[P(t) if t is not None else None for t in ts])


def u32(v):
    return (ctypes.c_uint32 * len(v))(*v)


def pack(cuda, ws, shapes):
    """Device weights and ngp_ffmlp_pack images of networks (in_dim, hidden, nl)."""
    nat, lib, P = _nat()
    wd = [dev(w, cuda) for w in ws]
    imgs = [torch.zeros(int(lib.ngp_ffmlp_image_bytes(*s)), dtype=torch.uint8, device=cuda) for s in shapes]
    assert all(i.numel() > 0 for i in imgs)
    nat.check(lib.ngp_ffmlp_pack(len(ws), arr(wd), u32([s[0] for s in shapes]), u32([s[1] for s in shapes]),
                                 u32([s[2] for s in shapes]), arr(imgs), None), "pack")
    return wd, imgs


def pack_pair(cuda, w_sigma, w_color, nl, nlc):
    return pack(cuda, [w_sigma, w_color], [(nc.IN, nc.HID, nl), (nc.IN, nc.HID, nlc)])


def to_pair(x, cuda):
    return dev(nc.pair_major(x), cuda)


# ---- a. the one-launch forward ---------------------------------------------------

def run_forward(cuda, nets, nl, nlc, enc, dirs, count, scale):
    """ngp_nerf_forward, and ngp_nerf_sigma_forward + ngp_ffmlp_forward_rows, on
    the same inputs: two (h, sigma, color_in, color_out) tuples of sentinel-filled
    outputs."""
    nat, lib, P = _nat()
    (ws, wc), (im_s, im_c) = nets
    B = len(enc)
    encp, d, cnt = to_pair(enc, cuda), dev(dirs, cuda), count_of(count, cuda)
    outs = []
    for one in (True, False):
        h, sig, ci, co = sent16((B, 16), cuda), sent32((B,), cuda), sent16((B, 32), cuda), sent16((B, 16), cuda)
        if one:
            nat.check(lib.ngp_nerf_forward(P(encp), P(im_s), P(im_c), B, P(cnt), 64, nl, 64, nlc, P(h), P(sig), P(ci),
                                           P(d), scale, P(co), None), "nerf_forward")
        else:
            nat.check(lib.ngp_nerf_sigma_forward(P(encp), P(ws), P(im_s), B, P(cnt), 32, 64, nl, P(h), P(sig), P(ci),
                                                 P(d), scale, PAIR, None), "sigma_forward")
            nat.check(lib.ngp_ffmlp_forward_rows(P(ci), P(wc), P(im_c), B, P(cnt), 32, 16, 64, nlc, 0, fc.NONE, P(co),
                                                 None), "forward_rows")
        outs.append((h, sig, ci, co))
    torch.cuda.synchronize()
    return outs


def check_forward_stages(out, n, enc_ref_h, dirs, w_color, nlc, scale, me_h, me_c, what):
    """Rows [0, n) of one forward against the oracle, stage by stage; rows past
    n keep their sentinels. Returns the device arrays and the largest errors."""
    h, sig, ci, co = out
    for t in out:
        assert kept(t[n:]), what
    h, sig, ci, co = host(h)[:n], host(sig)[:n], host(ci)[:n], host(co)[:n]
    eq_h = nc.close16(h, enc_ref_h[:n], f"{what} h", min_equal=me_h)
    np.testing.assert_allclose(sig, nc.sigma_of(h[:, 0], scale), rtol=1e-6, err_msg=what)
    ci_ref = nc.color_in_of(h, dirs[:n])
    assert np.array_equal(ci[:, 16:].view(np.uint16), ci_ref[:, 16:].view(np.uint16)), what  # geo columns and the pad
    nc.close16(ci, ci_ref, f"{what} color_in", min_equal=0.999)
    co_ref = nc.color_net(ci, w_color, nlc)
    eq_c = nc.close16(co, co_ref, f"{what} color_out", min_equal=me_c)
    err = lambda a, b: float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if n else 0.0  # noqa: E731
    return (h, co, co_ref), (err(h, enc_ref_h[:n]), eq_h, err(co, co_ref), eq_c)


@pytest.mark.parametrize("nl,nlc", nc.FWD_PAIRS)
def test_forward_every_depth_pair(cuda, parity_report, nl, nlc):
    """a. B in {1, 15, 33, 127, 257} with no count (the density scales in turn),
    each batch on its own and the pooled rows held to the rule (the batches
    below 257 rows with the share of their pooled rows); then 300
    allocated rows with count 173 at every density scale, and counts 0 and -3."""
    pool = nc.forward_pool(nl, nlc)
    pool.check_ranges()
    c0 = pool.cases[0]
    nets = pack_pair(cuda, c0.w_sigma, c0.w_color, nl, nlc)
    got, ref, worst = {"h": [], "co": []}, {"h": [], "co": []}, [0.0, 1.0, 0.0, 1.0]
    for k, c in enumerate(pool.cases):
        scale = nc.SCALES[k % 3]
        one, two = run_forward(cuda, nets, nl, nlc, c.enc, c.dirs, None, scale)
        for a, b in zip(one, two):
            assert same_bits(a, b), (c.B, "one launch != two launches")
        src = pool if nc.is_small(c.B) else c   # a few rows: the pooled share; 257 rows: the batch's own
        (h, co, co_ref), e = check_forward_stages(
            one, c.B, c.h, c.dirs, c.w_color, nlc, scale, src.min_equal("h"),
            src.min_equal("color_out"), f"B={c.B}")
        got["h"].append(h), got["co"].append(co), ref["h"].append(c.h), ref["co"].append(co_ref)
        worst = [max(worst[0], e[0]), min(worst[1], e[1]), max(worst[2], e[2]), min(worst[3], e[3])]
    nc.close16(np.concatenate(got["h"]), np.concatenate(ref["h"]), "pooled h", min_equal=pool.min_equal("h"))
    nc.close16(np.concatenate(got["co"]), np.concatenate(ref["co"]), "pooled color_out",
               min_equal=pool.min_equal("color_out"))
    B, n = nc.FWD_COUNTED
    c = nc.case(nl, nlc, B)
    c.check_ranges()
    enc, dirs = nan_from(c.enc, n), nan_from(c.dirs, n)
    for scale in nc.SCALES:
        one, two = run_forward(cuda, nets, nl, nlc, enc, dirs, n, scale)
        for a, b in zip(one, two):
            assert same_bits(a, b), (scale, "one launch != two launches")
        _, e = check_forward_stages(one, n, c.h, c.dirs, c.w_color, nlc, scale, c.min_equal("h"),
                                    c.min_equal("color_out"), f"count {n} of {B}, scale {scale}")
        worst = [max(worst[0], e[0]), min(worst[1], e[1]), max(worst[2], e[2]), min(worst[3], e[3])]
    for count in (0, -3):
        for out in run_forward(cuda, nets, nl, nlc, nan_from(c.enc, 0), nan_from(c.dirs, 0), count, 1.0):
            assert all(kept(t) for t in out), count
    parity_report(f"ngp_nerf_forward {nl}/{nlc}: max |d h| {worst[0]:.2e} (>= {worst[1]:.4f} bit-identical), "
                  f"max |d color_out| {worst[2]:.2e} (>= {worst[3]:.4f})")


def test_forward_past_grid_cap(cuda, parity_report):
    """a. 262 311 rows: 2048 workgroups, the first waves take a second chunk
    whose encodings and directions the first one's loop prefetched."""
    nl, nlc = nc.PAIR_FWD_STRIDE
    c = nc.case(nl, nlc, fc.B_FWD_STRIDE)
    c.check_ranges()
    nets = pack_pair(cuda, c.w_sigma, c.w_color, nl, nlc)
    one, two = run_forward(cuda, nets, nl, nlc, c.enc, c.dirs, None, 0.5)
    for a, b in zip(one, two):
        assert same_bits(a, b)
    _, e = check_forward_stages(one, c.B, c.h, c.dirs, c.w_color, nlc, 0.5, c.min_equal("h"),
                                c.min_equal("color_out"), f"B={c.B}")
    parity_report(f"ngp_nerf_forward {nl}/{nlc} B={c.B}: max |d h| {e[0]:.2e} ({e[1]:.4f} bit-identical), "
                  f"max |d color_out| {e[2]:.2e} ({e[3]:.4f})")


# ---- b. epilogue edges -------------------------------------------------------------

def check_edge_outputs(h, dirs, sig, ci, what):
    with np.errstate(over="ignore"):
        np.testing.assert_allclose(sig, nc.sigma_of(h[:, 0], 1.0), rtol=1e-6, err_msg=what)
    assert sig[0] == 0.0 and np.isinf(sig[len(nc.H0_EDGE) - 1]) and np.isfinite(sig[len(nc.H0_EDGE) - 2]), what
    ref = nc.color_in_of(h, dirs)
    assert np.array_equal(ci[:, 16:].view(np.uint16), ref[:, 16:].view(np.uint16)), what
    nc.close16(ci[:, :16], ref[:, :16], f"{what} SH", min_equal=0.999)


def test_glue_forward_edges(cuda):
    """b. ngp_nerf_glue_forward on the crafted rows: sigma is the float64 value
    cast to float32 (0 at -65504, finite at 88, infinity at 89), the geo
    columns are h's bits, the SH of the off-sphere directions is finite."""
    nat, lib, P = _nat()
    h, dirs, _ = nc.edge_h()
    R, B = len(h), len(h) + 7
    hd = dev(nan_from(np.concatenate([h, np.zeros((7, 16), np.float16)]), R), cuda)
    dd = dev(nan_from(np.concatenate([dirs, np.zeros((7, 3), np.float32)]), R), cuda)
    sig, ci = sent32((B,), cuda), sent16((B, 32), cuda)
    cnt = count_of(R, cuda)
    nat.check(lib.ngp_nerf_glue_forward(P(hd), P(dd), 1.0, P(sig), P(ci), B, P(cnt), None), "glue")
    torch.cuda.synchronize()
    assert kept(sig[R:]) and kept(ci[R:])
    check_edge_outputs(h, dirs, host(sig)[:R], host(ci)[:R], "glue")


def test_forward_edges_through_crafted_sigma_net(cuda):
    """b. The same h through ngp_nerf_forward: a sigma network whose last layer
    takes differences of the (non-negative) inputs gives the crafted h exactly
    (at most one non-zero term per sum). h must come out bit for bit, sigma
    and color_in as the glue's; the colour network runs on the device's
    color_in wherever that keeps it finite (the +-65504 geo rows overflow fp16
    in the oracle too), and equals the split launches wherever they are finite."""
    nl, nlc = nc.PAIR_EDGE
    h, dirs, n0 = nc.edge_h()
    enc, w_sigma = nc.crafted_sigma_net(h, nl)
    w_color = nc.make_weights(nl, nlc)[1]
    nets = pack_pair(cuda, w_sigma, w_color, nl, nlc)
    R = len(h)
    encn = nan_from(np.concatenate([enc, np.zeros((5, 32), np.float16)]), R)
    dirn = nan_from(np.concatenate([dirs, np.zeros((5, 3), np.float32)]), R)
    one, two = run_forward(cuda, nets, nl, nlc, encn, dirn, R, 1.0)
    for t in one:
        assert kept(t[R:])
    hd, sig, ci, co = (host(t)[:R] for t in one)
    assert np.array_equal(hd.view(np.uint16), h.view(np.uint16))
    check_edge_outputs(h, dirs, sig, ci, "one launch")
    for a, b in zip(one[:3], two[:3]):
        assert same_bits(a, b)
    co2 = host(two[3])[:R]
    fin = np.isfinite(co2.astype(np.float32))
    assert fin[:n0].all() and np.array_equal(fin, np.isfinite(co.astype(np.float32)))
    assert np.array_equal(co.view(np.uint16)[fin], co2.view(np.uint16)[fin])
    sub = np.abs(h.astype(np.float64)).max(-1) < 100          # the h0 rows up to 89 and the subnormal geo rows
    sub[:n0] = True
    ref = nc.color_net(ci[sub], w_color, nlc)
    assert np.isfinite(ref.astype(np.float64)).all() and sub.sum() == n0 + 30
    nc.close16(co[sub], ref, "edge color_out", min_equal=0.98)


@pytest.mark.parametrize("B,count", [(1, None), (255, None), (256, 256), (257, None), (600, 257), (600, 0), (600, -1)])
def test_glue_backward_edges(cuda, B, count):
    """b. Columns 1..15 from columns 16..30, column 0 kept, rows at or past the
    count untouched (256 threads per workgroup: one short of, at and past it)."""
    nat, lib, P = _nat()
    n = clip(B, count)
    r = np.random.default_rng([5, B, n])
    g = nan_from(r.standard_normal((B, 32)).astype(np.float16), n)
    g0 = r.standard_normal(B).astype(np.float16)
    gh = sent16((B, 16), cuda)
    gh[:, 0] = dev(g0, cuda)
    before = gh.clone()
    gd, cnt = dev(g, cuda), count_of(count, cuda)   # named: a tensor lives as long as the launch reads it
    nat.check(lib.ngp_nerf_glue_backward(P(gd), P(gh), B, P(cnt), None), "glue_bwd")
    torch.cuda.synchronize()
    assert same_bits(gh[n:], before[n:]) and same_bits(gh[:, 0], before[:, 0])
    assert np.array_equal(host(gh)[:n, 1:].view(np.uint16), np.ascontiguousarray(g[:n, 16:31]).view(np.uint16))


# ---- c, d. the one-launch backward -------------------------------------------------

def workspaces(cuda, B, nl, nlc, fill):
    _, lib, _ = _nat()
    return [torch.full((int(lib.ngp_ffmlp_backward_workspace_bytes(B, 32, 16, 64, k)),), fill, dtype=torch.uint8,
                       device=cuda) for k in (nl, nlc)]


def reduce_dw(cuda, wsb, B, nl, nlc, gw_dtype):
    """ngp_ffmlp_reduce of the (sigma, colour) workspaces: (dW sigma, dW colour)
    in NaN-filled buffers."""
    nat, lib, P = _nat()
    dt = torch.float16 if gw_dtype == F16 else torch.float32
    gw = [torch.full((nc.num_params(k),), float("nan"), dtype=dt, device=cuda) for k in (nl, nlc)]
    nat.check(lib.ngp_ffmlp_reduce(2, arr([wsb[1], wsb[0]]), u32([B, B]), u32([32, 32]), u32([64, 64]),
                                   u32([nlc, nl]), arr([gw[1], gw[0]]), gw_dtype, None, None), "reduce")
    return gw


def backward_inputs(cuda, g, cin, g_h0, enc, live):
    """Device inputs of a backward over the rows `live` (a count: rows [0, n); a
    row list: those rows): every other row is NaN. g_h starts as the sentinel
    with column 0 of the live rows given; g_enc as the sentinel."""
    B = len(g)
    mask = np.zeros(B, bool)
    if isinstance(live, int):
        mask[:live] = True
    else:
        mask[live] = True
    put = lambda a: dev(np.where(mask.reshape((-1,) + (1,) * (a.ndim - 1)), a, np.nan).astype(a.dtype), cuda)  # noqa: E731
    gh = sent16((B, 16), cuda)
    m = dev(mask, cuda)
    gh[m, 0] = dev(g_h0, cuda)[m]
    return put(g), put(cin), gh, to_pair(np.where(mask[:, None], enc, np.nan).astype(np.float16), cuda), \
        sent16((16, B, 2), cuda)


def one_launch_backward(cuda, nets, nl, nlc, inputs, B, count, rows=None, fill=7):
    """ngp_nerf_backward (rows None) or ngp_nerf_backward_live: (g_h, g_enc
    pair-major, workspaces)."""
    nat, lib, P = _nat()
    (_, _), (im_s, im_c) = nets
    go, ci, gh, encp, genc = inputs
    gh, genc = gh.clone(), genc.clone()
    wsb = workspaces(cuda, B, nl, nlc, fill)
    if rows is None:
        nat.check(lib.ngp_nerf_backward(P(go), P(ci), P(im_c), P(gh), P(encp), P(im_s), P(genc), B, P(count), 64, nl,
                                        64, nlc, P(wsb[0]), wsb[0].numel(), P(wsb[1]), wsb[1].numel(), None, None),
                  "nerf_backward")
    else:
        nat.check(lib.ngp_nerf_backward_live(P(go), P(ci), P(im_c), P(gh), P(encp), P(im_s), P(genc), B, P(rows),
                                             P(count), 64, nl, 64, nlc, P(wsb[0]), wsb[0].numel(), P(wsb[1]),
                                             wsb[1].numel(), None, None), "nerf_backward_live")
    return gh, genc, wsb


def two_call_backward(cuda, nets, nl, nlc, inputs, B, count):
    """The colour backward with its geo epilogue, then the sigma backward on the
    pair-major encodings (ngp_ffmlp_backward_rows, dW deferred)."""
    nat, lib, P = _nat()
    (ws, wc), (im_s, im_c) = nets
    go, ci, gh, encp, genc = inputs
    gh, genc = gh.clone(), genc.clone()
    wsb = workspaces(cuda, B, nl, nlc, 7)
    nat.check(lib.ngp_ffmlp_backward_rows(P(go), P(ci), P(wc), P(im_c), B, P(count), 32, 16, 64, nlc, 0, P(gh), None,
                                          F16, GEO | DEFER, P(wsb[1]), wsb[1].numel(), None), "backward_rows geo")
    nat.check(lib.ngp_ffmlp_backward_rows(P(gh), P(encp), P(ws), P(im_s), B, P(count), 32, 16, 64, nl, 0, P(genc),
                                          None, F16, PAIR | DEFER, P(wsb[0]), wsb[0].numel(), None),
              "backward_rows pair")
    return gh, genc, wsb


def dw_close(a, b, what):
    """The existing one-launch test's bound between two summation orders of the
    same fp32 partials: 2^-10 relative plus 1e-6."""
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all(), what
    assert torch.all((a - b).abs() <= 2.0 ** -10 * b.abs() + 1e-6), (what, float((a - b).abs().max()))


def check_backward_rows(c, sel, gh, genc, gw16, gw32, me_geo, me_enc, what):
    """The rows `sel` (a count or a row list) of a backward against the oracle
    on those rows: g_h[:, 1:16] (column 0 kept), g_enc on the device's g_h, and
    both dW in fp16 and fp32. Returns the largest errors."""
    idx = np.arange(sel) if isinstance(sel, int) else sel
    g, cin, enc, g_h0 = c.g[idx], c.color_in[idx], c.enc[idx], c.g_h0[idx]
    gi_ref, gwc_ref = nc.color_backward(g, cin, c.w_color, c.nlc)
    mag_c = nc.backward_mag(g, cin, c.w_color, c.nlc)
    gh = host(gh)[idx]
    assert np.array_equal(gh[:, 0].view(np.uint16), g_h0.view(np.uint16)), what
    eq_g = nc.close16(gh[:, 1:], gi_ref[:, 16:31], f"{what} g_h[:, 1:16]", min_equal=me_geo, mag=mag_c[:, 16:31])
    ge = nc.row_major(host(genc))[idx]
    ge_ref, gws_ref = nc.sigma_backward(gh, enc, c.w_sigma, c.nl)
    mag_s = nc.backward_mag(gh, enc, c.w_sigma, c.nl)
    eq_e = nc.close16(ge, ge_ref, f"{what} g_enc", min_equal=me_enc, mag=mag_s)
    errs = [float(np.abs(gh[:, 1:].astype(np.float64) - gi_ref[:, 16:31].astype(np.float64)).max()),
            float(np.abs(ge.astype(np.float64) - ge_ref.astype(np.float64)).max())]
    for name, g16, g32, ref in (("sigma", gw16[0], gw32[0], gws_ref), ("colour", gw16[1], gw32[1], gwc_ref)):
        close16(host(g16), ref, f"{what} dW {name}", min_equal=fc.DW_MIN_EQUAL)
        g = host(g32).astype(np.float64)
        assert np.isfinite(g).all(), what
        scale = float(np.abs(ref).max())
        assert float(np.abs(g - ref).max()) <= 1e-3 * scale, (what, name, float(np.abs(g - ref).max()), scale)
        # the same fp32 sum, rounded once (ngp_reduce.h)
        assert float((g32.half().view(torch.int16) == g16.view(torch.int16)).float().mean()) >= 0.99, (what, name)
        errs.append(float(np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30)))
    return errs + [eq_g, eq_e], (gh[:, 1:], gi_ref[:, 16:31], mag_c[:, 16:31]), (ge, ge_ref, mag_s)


def run_counted_backward(cuda, nets, c, B, count):
    """One launch and two calls over rows [0, n) of case c (count None: all B):
    the checks between them; returns the one launch's outputs."""
    nl, nlc, n = c.nl, c.nlc, clip(B, count)
    inputs = backward_inputs(cuda, c.g, c.color_in, c.g_h0, c.enc, n)
    cnt = count_of(count, cuda)
    gh, genc, wsb = one_launch_backward(cuda, nets, nl, nlc, inputs, B, cnt)
    gw16, gw32 = reduce_dw(cuda, wsb, B, nl, nlc, F16), reduce_dw(cuda, wsb, B, nl, nlc, F32)
    gh2, genc2, wsb2 = two_call_backward(cuda, nets, nl, nlc, inputs, B, cnt)
    gw2 = reduce_dw(cuda, wsb2, B, nl, nlc, F16)
    torch.cuda.synchronize()
    assert same_bits(gh, gh2) and same_bits(genc, genc2), "one launch != two calls"
    assert kept(gh[n:]) and kept(genc[:, n:]) and same_bits(gh[:n, 0], inputs[2][:n, 0])
    for a, b, name in zip(gw16, gw2, ("sigma", "colour")):
        dw_close(a, b, f"dW {name}")
    return gh, genc, gw16, gw32


@pytest.mark.parametrize("nl,nlc", nc.BWD_PAIRS)
def test_backward_small_allocations(cuda, parity_report, nl, nlc):
    """c. B in {1, 17, 33, 65, 97, 129, 161} with no count: one or two workgroups
    with 1, 2, 3, 4, 3 + 2 and 3 + 3 chunks (both idle-copy cases, 2 and 4
    halves). Each batch on its own and the pooled rows are held to the rule
    with the share of the pooled rows."""
    pool = nc.backward_pool(nl, nlc)
    pool.check_ranges()
    c0 = pool.cases[0]
    nets = pack_pair(cuda, c0.w_sigma, c0.w_color, nl, nlc)
    worst, least, geo, enc = [0.0] * 4, [1.0, 1.0], [], []
    for c in pool.cases:
        gh, genc, gw16, gw32 = run_counted_backward(cuda, nets, c, c.B, None)
        e, g3, e3 = check_backward_rows(c, c.B, gh, genc, gw16, gw32, pool.min_equal("g_geo"),
                                        pool.min_equal("g_enc"), f"B={c.B}")
        worst, least = [max(a, b) for a, b in zip(worst, e)], [min(a, b) for a, b in zip(least, e[4:])]
        geo.append(g3), enc.append(e3)
    for parts, key, what in ((geo, "g_geo", "pooled g_h[:, 1:16]"), (enc, "g_enc", "pooled g_enc")):
        got, ref, mag = (np.concatenate([p[k] for p in parts]) for k in range(3))
        nc.close16(got, ref, what, min_equal=pool.min_equal(key), mag=mag)
    parity_report(f"ngp_nerf_backward {nl}/{nlc} B<=161: max |d g_h| {worst[0]:.2e}, max |d g_enc| {worst[1]:.2e}, "
                  f"dW rel sigma {worst[2]:.1e} colour {worst[3]:.1e}; bit-identical g_h >= {least[0]:.4f}, "
                  f"g_enc >= {least[1]:.4f}")


@pytest.mark.parametrize("count", nc.BWD_COUNTS)
@pytest.mark.parametrize("nl,nlc", nc.BWD_PAIRS)
def test_backward_counts_under_the_grid_cap(cuda, parity_report, nl, nlc, count):
    """c. 32 807 allocated rows (256 workgroups) with counts that leave the
    workgroups 1 / 2, 2 / 3, 3, 4 / 5, 0 / 1 and 0 chunks."""
    B = fc.B_BWD_STRIDE
    c = nc.case(nl, nlc, B, True)
    c.check_ranges()
    nets = pack_pair(cuda, c.w_sigma, c.w_color, nl, nlc)
    if count == 0:
        # nothing is read or written but the slab rows, which every workgroup
        # writes as zeros: the reduce gives the empty sum whatever the slabs held
        inputs = backward_inputs(cuda, c.g, c.color_in, c.g_h0, c.enc, 0)
        gh, genc, wsb = one_launch_backward(cuda, nets, nl, nlc, inputs, B, count_of(0, cuda))
        gw = reduce_dw(cuda, wsb, B, nl, nlc, F16) + reduce_dw(cuda, wsb, B, nl, nlc, F32)
        torch.cuda.synchronize()
        assert kept(gh) and kept(genc)
        assert all(bool((g == 0).all()) for g in gw)
        return
    gh, genc, gw16, gw32 = run_counted_backward(cuda, nets, c, B, count)
    e, _, _ = check_backward_rows(c, count, gh, genc, gw16, gw32, c.min_equal("g_geo"),
                                  c.min_equal("g_enc"), f"count {count}")
    parity_report(f"ngp_nerf_backward {nl}/{nlc} count {count} of {B}: max |d g_h| {e[0]:.2e}, max |d g_enc| "
                  f"{e[1]:.2e}, dW rel sigma {e[2]:.1e} colour {e[3]:.1e}; bit-identical g_h {e[4]:.4f}, g_enc {e[5]:.4f}")


@pytest.mark.parametrize("which", ["empty", "one", "all", "third", "mid_chunk"])
@pytest.mark.parametrize("nl,nlc", nc.BWD_PAIRS)
def test_backward_live_rows(cuda, parity_report, nl, nlc, which):
    """d. ngp_nerf_backward_live over a row list inside 32 807 rows: the listed
    rows against the oracle on the gathered rows (every unlisted row's inputs
    are NaN), the unlisted rows' gradients untouched, and dW against the
    all-row launch with the unlisted rows' output gradients set to zero. The
    reduce takes no live count, so the workspaces start zeroed: workgroups
    past ngp_reduce::live_slab_rows write nothing."""
    B = fc.B_BWD_STRIDE
    c = nc.case(nl, nlc, B, True)
    rows = nc.live_lists()[which]
    n = len(rows)
    nets = pack_pair(cuda, c.w_sigma, c.w_color, nl, nlc)
    inputs = backward_inputs(cuda, c.g, c.color_in, c.g_h0, c.enc, np.array(rows))
    rd = dev(rows, cuda) if n else torch.zeros(1, dtype=torch.int32, device=cuda)
    gh, genc, wsb = one_launch_backward(cuda, nets, nl, nlc, inputs, B, count_of(n, cuda), rows=rd, fill=0)
    gw16, gw32 = reduce_dw(cuda, wsb, B, nl, nlc, F16), reduce_dw(cuda, wsb, B, nl, nlc, F32)
    torch.cuda.synchronize()
    unlisted = np.ones(B, bool)
    unlisted[rows] = False
    um = dev(unlisted, cuda)
    assert kept(gh[um]) and kept(genc[:, um])
    if n == 0:
        assert all(bool((g == 0).all()) for g in gw16 + gw32)
        assert all(int(w.count_nonzero()) == 0 for w in wsb)   # no workgroup wrote a slab row
        return
    e, _, _ = check_backward_rows(c, np.array(rows), gh, genc, gw16, gw32, c.min_equal("g_geo"),
                                  c.min_equal("g_enc"), f"live {which}")
    # the all-row launch: finite inputs everywhere, zero output gradients on the unlisted rows
    listed = ~unlisted
    g0 = np.where(listed[:, None], c.g, 0).astype(np.float16)
    gh0 = np.where(listed, c.g_h0, 0).astype(np.float16)
    all_in = backward_inputs(cuda, g0, c.color_in, gh0, c.enc, B)
    _, _, wsa = one_launch_backward(cuda, nets, nl, nlc, all_in, B, None)
    gwa = reduce_dw(cuda, wsa, B, nl, nlc, F16)
    torch.cuda.synchronize()
    for a, b, name in zip(gw16, gwa, ("sigma", "colour")):
        dw_close(a, b, f"live {which} dW {name}")
    parity_report(f"ngp_nerf_backward_live {nl}/{nlc} {which} ({n} of {B} rows): max |d g_h| {e[0]:.2e}, "
                  f"max |d g_enc| {e[1]:.2e}, dW rel sigma {e[2]:.1e} colour {e[3]:.1e}; bit-identical g_h {e[4]:.4f}, "
                  f"g_enc {e[5]:.4f}")


# ---- e. ngp_nerf_sigma_forward on every shape --------------------------------------

def unit_dirs(B, seed):
    d = np.random.default_rng([6, seed]).standard_normal((B, 3))
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("in_dim,hidden,nl", fc.SHAPES_RELU)
def test_sigma_forward_every_shape(cuda, in_dim, hidden, nl):
    """e. Every shape check_shape admits (launch_fwd_nerf dispatches all 12
    instantiations; InPairMajor masks the columns past in_dim, so pair-major
    input is accepted at every width): row-major and pair-major, with and
    without a packed image, 270 allocated rows with count 257. All four equal
    ngp_ffmlp_forward_rows + ngp_nerf_glue_forward bit for bit, and h the
    oracle."""
    nat, lib, P = _nat()
    c = fc.case(in_dim, hidden, nl, fc.B_RELU, out_cols=fc.OUT_RELU)
    c.check_ranges()
    n, B = c.B, c.B + 13
    (w,), (img,) = pack(cuda, [c.w], [(in_dim, hidden, nl)])
    x = nan_from(np.concatenate([c.x, np.zeros((13, in_dim), np.float16)]), n)
    dirs = unit_dirs(B, in_dim + hidden + nl)
    xd, xp, dd, cnt = dev(x, cuda), to_pair(x, cuda), dev(nan_from(dirs, n), cuda), count_of(n, cuda)
    h0, s0, ci0 = sent16((B, 16), cuda), sent32((B,), cuda), sent16((B, 32), cuda)
    nat.check(lib.ngp_ffmlp_forward_rows(P(xd), P(w), None, B, P(cnt), in_dim, 16, hidden, nl, 0, fc.NONE, P(h0),
                                         None), "forward_rows")
    nat.check(lib.ngp_nerf_glue_forward(P(h0), P(dd), 0.5, P(s0), P(ci0), B, P(cnt), None), "glue")
    for inp, image, flags in ((xd, None, 0), (xd, img, 0), (xp, img, PAIR), (xp, None, PAIR)):
        h, s, ci = sent16((B, 16), cuda), sent32((B,), cuda), sent16((B, 32), cuda)
        nat.check(lib.ngp_nerf_sigma_forward(P(inp), P(w), P(image), B, P(cnt), in_dim, hidden, nl, P(h), P(s), P(ci),
                                             P(dd), 0.5, flags, None), "sigma_forward")
        torch.cuda.synchronize()
        what = (in_dim, hidden, nl, image is not None, flags)
        assert same_bits(h, h0) and same_bits(s, s0) and same_bits(ci, ci0), what
        assert kept(h[n:]) and kept(s[n:]) and kept(ci[n:]), what
    hh = host(h0)[:n]
    close16(hh, c.out, "sigma_forward h")
    np.testing.assert_allclose(host(s0)[:n], nc.sigma_of(hh[:, 0], 0.5), rtol=1e-6)
    nc.close16(host(ci0)[:n], nc.color_in_of(hh, dirs[:n]), "color_in", min_equal=0.999)


@pytest.mark.parametrize("in_dim,hidden,nl", [(32, 128, 2), (32, 16, 2), (24, 64, 2), (80, 64, 2), (0, 64, 2),
                                              (32, 64, 1), (32, 64, 5)])
@pytest.mark.parametrize("flags", [0, PAIR])
def test_sigma_forward_rejects_other_shapes(cuda, in_dim, hidden, nl, flags):
    """e. A shape outside check_shape returns NGP_ERR_UNSUPPORTED and writes
    nothing, in either layout."""
    _, lib, P = _nat()
    B = 64
    x = torch.zeros(B * 128, dtype=torch.float16, device=cuda)
    w = torch.zeros(128 * 128 * 8, dtype=torch.float16, device=cuda)
    d = torch.zeros(B, 3, device=cuda)
    h, s, ci = sent16((B, 16), cuda), sent32((B,), cuda), sent16((B, 32), cuda)
    rc = lib.ngp_nerf_sigma_forward(P(x), P(w), None, B, None, in_dim, hidden, nl, P(h), P(s), P(ci), P(d), 1.0,
                                    flags, None)
    torch.cuda.synchronize()
    assert rc == ERR_UNSUPPORTED and kept(h) and kept(s) and kept(ci)
    assert lib.ngp_last_error()


# ---- f. the density forward --------------------------------------------------------

def density_rows_reference(cuda, c, w, scale):
    """h0 of ngp_ffmlp_forward_rows on the same values in row-major (device),
    and float32(scale * exp(h0))."""
    nat, lib, P = _nat()
    in_dim, hidden, nl = c.dims
    out = sent16((c.B, 16), cuda)
    x = dev(c.x, cuda)
    nat.check(lib.ngp_ffmlp_forward_rows(P(x), P(w), None, c.B, None, in_dim, 16, hidden, nl, 0, fc.NONE,
                                         P(out), None), "forward_rows")
    torch.cuda.synchronize()
    h0 = host(out)[:, 0]
    return h0, nc.sigma_of(h0, scale)


def check_density(sig, h0_dev, c, scale, what):
    """sig [B] against float32(scale * exp(h0)) of the device's own h0 (rtol
    1e-6), and against the oracle's h0: 98 % of the rows within rtol 1e-6
    (a batch below 257 rows, where one row is 3 % or more, is held to that over
    the pooled rows of its group by the caller) and every row's
    log(sigma / scale) within close16's tolerance of it. Returns the rows'
    within-1e-6 mask."""
    np.testing.assert_allclose(sig, nc.sigma_of(h0_dev, scale), rtol=1e-6, err_msg=what)
    ref_h0 = c.out[:, 0]
    ref = nc.sigma_of(ref_h0, scale).astype(np.float64)
    within = np.abs(sig - ref) <= 1e-6 * np.abs(ref)
    if not nc.is_small(c.B):
        assert within.mean() >= 0.98, (what, float(within.mean()))
    r = ref_h0.astype(np.float64)
    tol = 2 * np.spacing(np.abs(ref_h0)).astype(np.float64) + 1e-3 * np.abs(r).max()
    assert (np.abs(np.log(sig.astype(np.float64) / scale) - r) <= tol).all(), what
    return within


def scatter_indices(B, seed):
    """Cell indices with duplicates, gaps and a permutation: B rows into
    B + 40 cells, every fifth row onto its predecessor's cell."""
    r = np.random.default_rng([8, B, seed])
    idx = r.permutation(B + 40)[:B].astype(np.int32)
    idx[4::5] = idx[3::5][:len(idx[4::5])]
    return idx


def check_scatter(grid, idx, rows_sig, what):
    """Each touched cell holds the bitwise maximum of its rows' densities (they
    are >= 0, so the float and the integer order agree); the others keep -1."""
    want = np.full(grid.shape, -1.0, np.float32)
    np.maximum.at(want, idx, rows_sig)
    assert np.array_equal(grid.view(np.uint32), want.view(np.uint32)), what
    assert (grid[np.setdiff1d(np.arange(len(grid)), idx)] == -1.0).all()


@pytest.mark.parametrize("hidden,nl", nc.DENSITY_SHAPES)
def test_density_forward_streaming_shapes(cuda, parity_report, hidden, nl):
    """f. k_density_fwd<W, NH> (32 inputs, packed image): per row and scattered,
    B in {1, 31, 33, 257}; density_scale 0 leaves 0.0 in the touched cells.
    The 257-row batch on its own and the 322 pooled rows of the four batches
    have 98 % of their rows within 1e-6 of the oracle's density."""
    nat, lib, P = _nat()
    worst, pooled = 1.0, {1.0: [], 0.5: []}
    for B in nc.B_DENSITY:
        c = fc.case(32, hidden, nl, B, backward=False)
        c.check_ranges(pooled=True)
        (w,), (img,) = pack(cuda, [c.w], [c.dims])
        xp = to_pair(c.x, cuda)
        h0, _ = density_rows_reference(cuda, c, w, 1.0)
        idx = scatter_indices(B, hidden + nl)
        idx_d = dev(idx, cuda)
        for scale in (1.0, 0.5, 0.0):
            sig = sent32((B + 3,), cuda)
            nat.check(lib.ngp_nerf_density_forward_rows(P(xp), P(img), B, hidden, nl, scale, P(sig), None), "rows")
            grid = torch.full((B + 40,), -1.0, device=cuda)
            nat.check(lib.ngp_nerf_density_forward(P(xp), P(w), P(img), B, 32, hidden, nl, scale, P(idx_d),
                                                   P(grid), None), "scatter")
            torch.cuda.synchronize()
            assert kept(sig[B:])
            s = host(sig)[:B]
            if scale:
                within = check_density(s, h0, c, scale, f"{c.dims} B={B} scale {scale}")
                pooled[scale].append(within)
                worst = min(worst, float(within.mean()))
            else:
                assert (s.view(np.uint32) == 0).all()
            check_scatter(host(grid), idx, s, (c.dims, B, scale))
    share = min(float(np.concatenate(w).mean()) for w in pooled.values())
    assert share >= 0.98, (hidden, nl, share)
    parity_report(f"ngp_nerf_density_forward_rows <{hidden}, {nl - 1}>: {share:.4f} of the pooled rows within 1e-6 of "
                  f"the oracle's density (least batch {worst:.4f})")


@pytest.mark.parametrize("in_dim,hidden,nl", fc.SHAPES_RELU)
def test_density_forward_without_image(cuda, in_dim, hidden, nl):
    """f. No image: k_mlp_fwd with EpiDensity on pair-major input of width
    in_dim, the weights packed per workgroup."""
    nat, lib, P = _nat()
    c = fc.case(in_dim, hidden, nl, fc.B_RELU, out_cols=fc.OUT_RELU)
    w = dev(c.w, cuda)
    h0, want = density_rows_reference(cuda, c, w, 0.5)
    idx = np.random.default_rng([9, in_dim, hidden, nl]).permutation(c.B + 9)[:c.B].astype(np.int32)
    grid = torch.full((c.B + 9,), -1.0, device=cuda)
    xp, idx_d = to_pair(c.x, cuda), dev(idx, cuda)
    nat.check(lib.ngp_nerf_density_forward(P(xp), P(w), None, c.B, in_dim, hidden, nl, 0.5, P(idx_d), P(grid), None),
              "density_forward")
    torch.cuda.synchronize()
    g = host(grid)
    check_density(g[idx], h0, c, 0.5, f"{c.dims} no image")
    check_scatter(g, idx, g[idx], c.dims)


@pytest.mark.parametrize("hidden,nl", [(64, 2), (32, 4)])
def test_density_forward_image_narrow_input(cuda, hidden, nl):
    """f. A 16-wide input with a packed image: IN_KS is 1 as for 32 inputs, but
    the streaming kernel reads 16 pairs per row, so launch_fwd_density keeps
    the generic kernel for it. The 8 pairs lie at the head of a 16-pair buffer
    whose tail is NaN: a kernel that reads past pair 8 meets NaN (times the
    image's zero padding) instead of memory beyond the input."""
    nat, lib, P = _nat()
    c = fc.case(16, hidden, nl, fc.B_RELU, out_cols=fc.OUT_RELU)
    (w,), (img,) = pack(cuda, [c.w], [c.dims])
    h0, _ = density_rows_reference(cuda, c, w, 1.0)
    buf = torch.full((16, c.B, 2), float("nan"), dtype=torch.float16, device=cuda)
    buf[:8] = to_pair(c.x, cuda)
    idx = np.arange(c.B, dtype=np.int32)[::-1].copy()
    idx_d = dev(idx, cuda)
    grids = []
    for image in (img, None):
        grid = torch.full((c.B,), -1.0, device=cuda)
        nat.check(lib.ngp_nerf_density_forward(P(buf), P(w), P(image), c.B, 16, hidden, nl, 1.0, P(idx_d),
                                               P(grid), None), "density_forward")
        grids.append(grid)
    torch.cuda.synchronize()
    assert same_bits(grids[0], grids[1])
    check_density(host(grids[0])[idx], h0, c, 1.0, f"{c.dims} image")


def test_density_forward_past_grid_cap(cuda, parity_report):
    """f. 262 311 rows: more chunks than 2048 resident workgroups hold, so every
    wave of k_density_fwd streams (its prefetch of the chunk one stride ahead
    included), and k_mlp_fwd's grid-stride loop runs in the scattered form."""
    nat, lib, P = _nat()
    c = fc.case(*fc.SHAPE_EDGE, fc.B_FWD_STRIDE, 0, backward=False)
    in_dim, hidden, nl = c.dims
    (w,), (img,) = pack(cuda, [c.w], [c.dims])
    xp = to_pair(c.x, cuda)
    h0, _ = density_rows_reference(cuda, c, w, 1.0)
    sig = sent32((c.B,), cuda)
    nat.check(lib.ngp_nerf_density_forward_rows(P(xp), P(img), c.B, hidden, nl, 1.0, P(sig), None), "rows")
    idx = scatter_indices(c.B, 0)
    idx_d = dev(idx, cuda)
    grids = []
    for image in (img, None):
        grid = torch.full((c.B + 40,), -1.0, device=cuda)
        nat.check(lib.ngp_nerf_density_forward(P(xp), P(w), P(image), c.B, in_dim, hidden, nl, 1.0, P(idx_d),
                                               P(grid), None), "scatter")
        grids.append(grid)
    torch.cuda.synchronize()
    s = host(sig)
    share = float(check_density(s, h0, c, 1.0, f"B={c.B}").mean())
    for grid in grids:
        check_scatter(host(grid), idx, s, c.B)
    parity_report(f"ngp_nerf_density_forward_rows B={c.B}: {share:.4f} of the rows within 1e-6 of the oracle's density")


# ---- g. the trainer's gates ----------------------------------------------------------

def _trainer(cuda, nl, nlc, options=None):
    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10, num_layers=nl, num_layers_color=nlc).to(cuda)
    with torch.no_grad():
        model.encoder.embeddings.normal_(0, 0.05)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield(cascade=model.cascade, bound=1.0)).to(cuda))
    data = SyntheticLego(cuda, num_rays=256)
    return model, data, FusedTrainer(model, data, M=16384, seed=3, dt_gamma=0.0, options=options)


@pytest.mark.parametrize("nl,nlc,one_bwd", [(3, 2, True), (2, 4, False)])
def test_trainer_gates_take_the_one_launch_paths(cuda, nl, nlc, one_bwd):
    """g. NeRFNetwork(num_layers, num_layers_color) through FusedTrainer: (3, 2)
    takes ngp_nerf_forward and ngp_nerf_backward, (2, 4) the forward only (the
    backward has no 4-layer colour instantiation). One _forward_backward
    against split_fwd / split_bwd: h, sigma, color_in, color_out and the
    encoding gradients bit for bit, the MLP gradients within the bound between
    two summation orders."""
    outs = []
    for split in (False, True):
        _, _, ft = _trainer(cuda, nl, nlc, dict(split_fwd=split, split_bwd=split))
        assert ft._one_fwd == (not split) and ft._one_bwd == (one_bwd and not split)
        ft._sample()
        ft._forward_backward()
        torch.cuda.synchronize()
        n = int(ft.counter[0])
        assert 0 < n <= ft.M
        genc = ft.g_enc.view(16, ft.M, 2)[:, :n]
        outs.append((n, [ft.h_sigma[:n].clone(), ft.sigma[:n].clone(), ft.color_in[:n].clone(),
                         ft.color_out[:n].clone(), genc.clone()], [g.clone() for g in ft.grads]))
    (n0, a, ga), (n1, b, gb) = outs
    assert n0 == n1
    for name, x, y in zip(["h", "sigma", "color_in", "color_out", "g_enc"], a, b):
        assert torch.isfinite(x.float()).all() and same_bits(x, y), name
    assert same_bits(ga[0], gb[0])   # the table gradient: exact bin sums of identical g_enc
    for x, y, name in zip(ga[1:3], gb[1:3], ("sigma", "colour")):
        assert float(x.float().abs().max()) > 0
        dw_close(x, y, f"trainer dW {name}")


def test_fused_render_on_a_three_two_network(cuda, parity_report):
    """g. FusedRenderer on NeRFNetwork(num_layers=3, num_layers_color=2) against
    the reference inference loop, with tests/test_gpu_render.py's tolerance."""
    from nerf.fused_render import FusedRenderer
    from test_gpu_render import _compare, _rays
    model, data, _ = _trainer(cuda, 3, 2)
    model.eval()
    H = W = 64
    ro, rd = _rays(data, H, W)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ref = model.render(ro, rd, staged=True, bg_color=1, perturb=False, dt_gamma=0.0, max_steps=1024)
    r = FusedRenderer(model, H * W, dt_gamma=0.0)
    r.load_weights()
    r.capture()
    got = r.render(ro, rd, bg_color=1)
    torch.cuda.synchronize()
    assert float(got["weights_sum"].max()) > 0
    frac, dmax = _compare(ref, got, "3/2 network")
    parity_report(f"fused render 3/2 network {W}x{H}: {frac:.5f} of pixels within 1e-3, max |d| {dmax:.2e}")
