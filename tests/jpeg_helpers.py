"""Shared by the JPEG / video tests: a reference baseline JPEG encoder and
decoder in numpy float64 and pure Python, written from ITU-T T.81 (and the JFIF
colour conversion) apart from nerf/jpeg.py and csrc/jpeg.hip on purpose, and the
images the tests run.

  ref_coefficients  A.3.3 (FDCT), A.3.4 (quantisation), Figure A.6 (zigzag)
  ref_scan          F.1.2 (Huffman coding of DC differences and AC run/size),
                    Annex C (codes from BITS / HUFFVAL), B.1.1.5 (byte stuffing),
                    E.1.4 / F.1.2.3 (restart intervals, padding with 1 bits)
  ref_decode        the inverse of ref_coefficients, float64 until the last step

PIL (libjpeg) is the independent judge of the files; the two bounds below were
measured with it by tests/test_jpeg_cpu.py, which prints the figures.
"""
import io

import numpy as np

# ---- bounds measured against PIL's decoder (tests/test_jpeg_cpu.py) ----
# max |PIL decode - ref_decode| over every case below, in grey levels. PIL's
# libjpeg uses an integer IDCT (13-bit constants) and, for colour, a fixed-point
# YCbCr -> RGB table (16-bit constants) after rounding Y, Cb, Cr to integers;
# ref_decode rounds once at the end. Measured: grey 1, colour 2.
DECODE_BOUND = {1: 1, 3: 2}
# PSNR against the source: PIL's own encoding with the same tables (qtables=,
# subsampling=0) minus the reference encoder's file, both decoded by PIL, in dB,
# the largest over PSNR_CASES. PIL's encoder uses an integer DCT, the reference
# float64; on a ramp, where a handful of coefficients decide, either can come out
# ahead. Measured: 0.3357 dB (colour vertical ramp 20 x 28 at quality 50: PIL
# 36.523 dB, the reference 36.187 dB).
PSNR_GAP_MEASURED = 0.336
PSNR_MARGIN = PSNR_GAP_MEASURED + 0.1

SHAPES = [(1, 1), (8, 8), (9, 17), (20, 28), (80, 8), (8, 520), (64, 64)]

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
          14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
          46, 53, 60, 61, 54, 47, 55, 62, 63]

# Annex K.3 (BITS, HUFFVAL): Tables K.3, K.4 (DC luminance, chrominance), K.5, K.6 (AC)
_K3 = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
_K4 = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
_K5 = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], list(bytes.fromhex(
    "01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72"
    "82 09 0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59"
    "5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3"
    "a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2"
    "e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa")))
_K6 = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], list(bytes.fromhex(
    "00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1"
    "0a 16 24 34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58"
    "59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a"
    "a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da"
    "e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa")))


def _codes(bits, vals):
    """Annex C: symbol -> (code, length). Codes of one length are consecutive;
    going to the next length appends a 0 bit."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (_codes(*_K3), _codes(*_K4))
AC_CODES = (_codes(*_K5), _codes(*_K6))

# A.3.3: S(v, u) = 1/4 C(u) C(v) sum s(y, x) cos((2x+1) u pi / 16) cos((2y+1) v pi / 16) = (D s D^T)(v, u)
_D = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) * 0.5 * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)]
               for u in range(8)])


def _planes(image):
    """uint8 [H, W] or [H, W, 3] -> float64 level-shifted component planes, edges repeated to multiples of 8."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    pad = ((0, -H % 8), (0, -W % 8)) + (((0, 0),) if image.ndim == 3 else ())
    x = np.pad(image, pad, mode="edge").astype(np.float64)
    if image.ndim == 2:
        return [x - 128.0]
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    return [(0.299 * R + 0.587 * G + 0.114 * B) - 128.0,
            (-0.168736 * R - 0.331264 * G + 0.5 * B + 128.0) - 128.0,
            (0.5 * R - 0.418688 * G - 0.081312 * B + 128.0) - 128.0]


def ref_coefficients(image, tables):
    """-> (coefs int64 [blocks, 64], quotients float64 [blocks, 64]): zigzag
    order, blocks in MCU order (row of MCUs, MCU, component). quotients are
    S / Q before rounding; coefs = rint, DC clamped to +-2047, AC to +-1023."""
    planes = _planes(image)
    comps = len(planes)
    my, mx = planes[0].shape[0] // 8, planes[0].shape[1] // 8
    quot = np.zeros((my * mx * comps, 64))
    for c, plane in enumerate(planes):
        q = np.asarray(tables[0 if c == 0 else 1], dtype=np.float64).reshape(8, 8)
        blocks = plane.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3)  # [my, mx, y, x]
        S = np.einsum("vy,abyx,ux->abvu", _D, blocks, _D) / q
        quot[c::comps] = S.reshape(my * mx, 64)[:, ZIGZAG]
    coefs = np.rint(quot).astype(np.int64)
    coefs[:, 0] = np.clip(coefs[:, 0], -2047, 2047)
    coefs[:, 1:] = np.clip(coefs[:, 1:], -1023, 1023)
    return coefs, quot


def _magnitude(v):
    """F.1.2.1: (category SSSS, the SSSS low bits of v, or of v - 1 if v < 0)."""
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def ref_scan(coefs, H, W, components, symbols=None):
    """The entropy-coded segment of coefs [blocks, 64] (zigzag, MCU order) with a
    restart interval of one MCU row: DC predictors reset per interval, each
    interval padded with 1 bits and byte-stuffed, RSTm (m = 0..7 cycling)
    between intervals. symbols: a list that receives every Huffman symbol."""
    mx, my = (W + 7) // 8, (H + 7) // 8
    coefs = np.asarray(coefs).reshape(my, mx, components, 64).tolist()
    out = bytearray()
    for row in range(my):
        acc, nbits = 0, 0
        pred = [0] * components
        for m in range(mx):
            for c in range(components):
                t = 0 if c == 0 else 1
                zz = coefs[row][m][c]
                size, extra = _magnitude(zz[0] - pred[c])
                pred[c] = zz[0]
                code, length = DC_CODES[t][size]
                items = [(code, length), (extra, size)]
                if symbols is not None:
                    symbols.append(size)
                run = 0
                for k in range(1, 64):
                    if zz[k] == 0:
                        run += 1
                        continue
                    while run > 15:
                        items.append(AC_CODES[t][0xF0])
                        if symbols is not None:
                            symbols.append(0xF0)
                        run -= 16
                    size, extra = _magnitude(zz[k])
                    items += [AC_CODES[t][(run << 4) | size], (extra, size)]
                    if symbols is not None:
                        symbols.append((run << 4) | size)
                    run = 0
                if run:
                    items.append(AC_CODES[t][0x00])
                    if symbols is not None:
                        symbols.append(0x00)
                for value, length in items:
                    acc = (acc << length) | value
                    nbits += length
        pad = -nbits % 8
        acc = (acc << pad) | ((1 << pad) - 1)
        data = acc.to_bytes((nbits + pad) // 8, "big")
        out += data.replace(b"\xff", b"\xff\x00")
        if row + 1 < my:
            out += bytes([0xFF, 0xD0 + (row & 7)])
    return bytes(out)


def ref_decode(coefs, H, W, components, tables):
    """coefs [blocks, 64] -> uint8 [H, W] or [H, W, 3]: dequantise, inverse DCT,
    level shift and clamp to 0..255 per component, inverse JFIF conversion, all in
    float64; one rounding at the end."""
    mx, my = (W + 7) // 8, (H + 7) // 8
    coefs = np.asarray(coefs, dtype=np.float64).reshape(my * mx, components, 64)
    planes = []
    for c in range(components):
        q = np.asarray(tables[0 if c == 0 else 1], dtype=np.float64).reshape(64)
        nat = np.zeros((my * mx, 64))
        nat[:, ZIGZAG] = coefs[:, c]
        S = (nat * q).reshape(my, mx, 8, 8)
        s = np.einsum("vy,abvu,ux->abyx", _D, S, _D)
        # A.3.1: the level-shifted output is clamped to the sample range, component by component
        planes.append(np.clip(s.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)[:H, :W] + 128.0, 0.0, 255.0))
    if components == 1:
        x = planes[0]
    else:
        Y, Cb, Cr = planes[0], planes[1] - 128.0, planes[2] - 128.0
        x = np.stack([Y + 1.402 * Cr, Y - 0.344136 * Cb - 0.714136 * Cr, Y + 1.772 * Cb], axis=-1)
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


# ---- the images ----
def _grey(kind, H, W):
    if kind == "noise":
        return np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W)).astype(np.uint8)
    if kind == "hramp":
        return np.broadcast_to(np.linspace(0, 255, W).astype(np.uint8)[None, :], (H, W)).copy()
    if kind == "vramp":
        return np.broadcast_to(np.linspace(0, 255, H).astype(np.uint8)[:, None], (H, W)).copy()
    if kind.startswith("flat"):
        return np.full((H, W), int(kind[4:]), dtype=np.uint8)
    if kind == "checker":
        y, x = np.mgrid[:H, :W]
        return (((x + y) & 1) * 255).astype(np.uint8)
    if kind == "cos77":  # 128 + 60 cos of the (7, 7) basis function: only coefficient 63 survives quality 50
        y, x = np.mgrid[:H, :W]
        return np.rint(128 + 60 * np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) *
                       np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)).astype(np.uint8)
    raise ValueError(kind)


KINDS = ["noise", "hramp", "vramp", "flat0", "flat128", "flat255", "checker"]


def make_image(kind, H, W, components):
    """Grey: the pattern. Colour: the pattern in R, its transpose-like variants
    in G and B (noise: three draws), so that Cb and Cr are not flat; the flat
    images, the checkerboard and the basis function in all three (Y as in grey)."""
    g = _grey(kind, H, W)
    if components == 1:
        return g
    if kind == "noise":
        return np.random.default_rng(H * 1000 + W + 7).integers(0, 256, (H, W, 3)).astype(np.uint8)
    if kind in ("hramp", "vramp"):
        return np.stack([g, g[::-1, ::-1], _grey("vramp" if kind == "hramp" else "hramp", H, W)], axis=-1)
    return np.stack([g, g, g], axis=-1)


def cases(H, W):
    """(kind, quality) the shape runs, with either component count: every image
    at quality 90; at (20, 28) and (64, 64) also at 50 and 100; the (7, 7) basis
    function at quality 50 where the shape is whole blocks; at (20, 28) noise at quality 1 (quantisers clamp at
    255)."""
    out = [(k, 90) for k in KINDS]
    if (H, W) in ((20, 28), (64, 64)):
        out += [(k, q) for q in (50, 100) for k in KINDS]
    if H % 8 == 0 and W % 8 == 0:  # (whole blocks only: edge padding would break the basis function)
        out.append(("cos77", 50))
    if (H, W) == (20, 28):
        out.append(("noise", 1))
    return out


PSNR_CASES = [(H, W, kind, q) for (H, W) in ((20, 28), (64, 64)) for kind in ("noise", "hramp", "vramp", "checker")
              for q in (50, 90, 100)]


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2))
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def pil_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def pil_encode(image, tables):
    """PIL's own baseline encoding with the given tables (natural order), 4:4:4."""
    from PIL import Image
    buf = io.BytesIO()
    tabs = [[int(v) for v in t] for t in tables]
    im = Image.fromarray(image)
    if image.ndim == 2:
        im.save(buf, "JPEG", qtables=tabs[:1])
    else:
        im.save(buf, "JPEG", qtables=tabs, subsampling=0)
    return buf.getvalue()
