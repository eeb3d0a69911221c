"""GPU: the device JPEG encoder (csrc/jpeg.hip, nerf/jpeg.py) against the
reference encoder of tests/jpeg_helpers.py and PIL.

Coefficients: the workspace equals rint of the float64 quotients; a difference
of +-1 is allowed only where the float64 quotient lies within 1e-3 of a
half-integer, on at most 2 % of an image's coefficients (float32 against
float64 DCT differs only at ties: 0 to 0.29 % of 64 x 64 noise, and 0.24 to
0.76 % of its coefficients lie in the band at all). Scan: the device's bytes
equal ref_scan of the device's own coefficients, byte for byte."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_helpers as jh

pytestmark = pytest.mark.gpu

GUARD = 64


def _encode_raw(cuda, image, quality):
    """The C entry on `image` with guard bytes behind the scan buffer ->
    (coefficients [blocks, 64], scan bytes, capacity, tables)."""
    import _ngp_native as nat
    from nerf import jpeg
    H, W = image.shape[:2]
    comps = 1 if image.ndim == 2 else 3
    lib, P = nat.lib(), nat.ptr
    tables = jpeg.quant_tables(quality)
    q = [(ctypes.c_uint16 * 64)(*[int(v) for v in t]) for t in tables]
    capacity = lib.ngp_jpeg_scan_capacity(H, W, comps)
    blocks = ((H + 7) // 8) * ((W + 7) // 8) * comps
    ws = torch.full((lib.ngp_jpeg_workspace_elems(H, W, comps),), 12345, dtype=torch.int16, device=cuda)
    out = torch.full((capacity + GUARD,), 0xA5, dtype=torch.uint8, device=cuda)
    out_len = torch.full((1,), -1, dtype=torch.int32, device=cuda)
    pixels = torch.from_numpy(image).to(cuda).contiguous()
    nat.check(lib.ngp_jpeg_encode(P(pixels), H, W, comps, q[0], q[1] if comps == 3 else None, P(ws), P(out), capacity,
                                  P(out_len), nat.stream_of(out)), "jpeg_encode")
    torch.cuda.synchronize()
    n = int(out_len.item())
    assert 0 < n <= capacity, (n, capacity)
    host = out.cpu().numpy()
    assert (host[capacity:] == 0xA5).all(), "bytes past capacity were written"
    assert (host[n:capacity] == 0xA5).all(), "bytes past the scan's length were written"
    return ws[:blocks * 64].view(blocks, 64).cpu().numpy().astype(np.int64), host[:n].tobytes(), capacity, tables


def _check_coefficients(got, image, tables, what):
    want, quot = jh.ref_coefficients(image, tables)
    diff = got - want
    off = diff != 0
    share = float(off.mean())
    if off.any():
        assert np.abs(diff[off]).max() == 1, (what, "a coefficient is off by more than 1")
        from_half = np.abs(np.abs(quot[off] - np.floor(quot[off])) - 0.5)
        assert from_half.max() < 1e-3, (what, "a coefficient differs away from a tie", float(from_half.max()))
    assert share <= 0.02, (what, share)
    return share


@pytest.mark.parametrize("comps", [1, 3])
@pytest.mark.parametrize("shape", jh.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coefficients_and_scan(cuda, shape, comps, parity_report):
    H, W = shape
    worst = 0.0
    for kind, quality in jh.cases(H, W):
        what = (H, W, comps, kind, quality)
        image = jh.make_image(kind, H, W, comps)
        coefs, scan, capacity, tables = _encode_raw(cuda, image, quality)
        worst = max(worst, _check_coefficients(coefs, image, tables, what))
        want = jh.ref_scan(coefs, H, W, comps)
        assert len(scan) == len(want), (what, len(scan), len(want))
        assert scan == want, (what, next(i for i in range(len(want)) if scan[i] != want[i]))
    line = f"jpeg {H}x{W}x{comps}: largest share of coefficients off by one at a tie {worst:.5f}"
    print(line)
    parity_report(line)


def test_rgb_and_grey_share_nothing(cuda):
    """An [H, W, 3] image whose channels are equal codes its Y blocks as the grey image's."""
    g = jh.make_image("noise", 20, 28, 1)
    grey, _, _, _ = _encode_raw(cuda, g, 90)
    colour, _, _, _ = _encode_raw(cuda, np.stack([g, g, g], axis=-1), 90)
    y = colour.reshape(-1, 3, 64)
    assert np.abs(y[:, 0] - grey).max() <= 1 and float((y[:, 0] != grey).mean()) <= 0.02
    assert not y[:, 1:].any()  # Cb = Cr = 128: nothing after the level shift


@pytest.mark.parametrize("comps", [1, 3])
def test_files_load_in_pil_and_match_its_encoder(cuda, comps, parity_report):
    from nerf.jpeg import JpegEncoder
    encoders = {}
    worst = -1e9
    for H, W, kind, quality in jh.PSNR_CASES:
        enc = encoders.setdefault((H, W, quality), JpegEncoder(H, W, comps, quality, cuda))
        image = jh.make_image(kind, H, W, comps)
        t = torch.from_numpy(image).to(cuda)
        data = enc.encode(t)
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        im = jh.pil_decode(data)
        assert im.size == (W, H) and im.mode == ("L" if comps == 1 else "RGB")
        ours = jh.psnr(np.asarray(im), image)
        theirs = jh.psnr(np.asarray(jh.pil_decode(jh.pil_encode(image, enc.tables))), image)
        gap = 0.0 if ours == theirs else theirs - ours
        worst = max(worst, gap)
        assert ours >= theirs - jh.PSNR_MARGIN, (H, W, comps, kind, quality, ours, theirs)
        # the decode is the float64 decode of the device's coefficients, as far as libjpeg's integers allow
        ref = jh.ref_decode(enc.coefficients().cpu().numpy(), H, W, comps, enc.tables)
        assert np.abs(np.asarray(im).astype(np.int32) - ref.astype(np.int32)).max() <= jh.DECODE_BOUND[comps]
        assert enc.encode(t) == data  # the same bytes again
        other = JpegEncoder(H, W, comps, quality, cuda)  # ... and from fresh buffers
        assert other.encode(t) == data
    line = f"jpeg files x{comps}: PIL's encoder ahead by at most {worst:.4f} dB (margin {jh.PSNR_MARGIN:.3f})"
    print(line)
    parity_report(line)


def test_submit_and_result_pipeline(cuda):
    from nerf.jpeg import JpegEncoder
    enc = JpegEncoder(20, 28, 3, 90, cuda)
    images = [torch.from_numpy(jh.make_image(k, 20, 28, 3)).to(cuda) for k in ("noise", "hramp", "checker")]
    alone = [enc.encode(t) for t in images]
    assert len(set(alone)) == 3
    got = []
    enc.submit(images[0])
    for t in images[1:]:
        enc.submit(t)
        got.append(enc.result())  # the image before: its copy is known to be done, no wait of its own
    got.append(enc.result())
    assert got == alone
    with pytest.raises(RuntimeError):
        enc.result()
    enc.submit(images[0])
    enc.submit(images[1])
    with pytest.raises(RuntimeError):
        enc.submit(images[2])
    assert [enc.result(), enc.result()] == alone[:2]
    with pytest.raises(ValueError):
        enc.encode(images[0][:8])
    with pytest.raises(RuntimeError):
        enc.encode(images[0].cpu())
