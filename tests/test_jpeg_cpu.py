"""CPU: the host half of the device JPEG encoder (nerf/jpeg.py) and the
reference encoder the GPU tests compare with (tests/jpeg_helpers.py), both
judged by PIL's libjpeg; the C entry's argument checks, which need no GPU."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

import jpeg_helpers as jh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pil_order():
    """'natural' or 'zigzag': the order of Image.quantization in this Pillow
    (natural since 8.3). At quality 50 libjpeg's luminance table is Annex K.1
    itself, whose third entry is 10 in natural order and 12 in zigzag order."""
    buf = io.BytesIO()
    Image.new("L", (8, 8)).save(buf, "JPEG", quality=50)
    t = Image.open(io.BytesIO(buf.getvalue())).quantization[0]
    assert (t[0], t[1]) == (16, 11) and t[2] in (10, 12)
    return "natural" if t[2] == 10 else "zigzag"


def _natural(table, order):
    table = list(table)
    if order == "natural":
        return table
    out = [0] * 64
    for k, n in enumerate(jh.ZIGZAG):
        out[n] = table[k]
    return out


@pytest.mark.parametrize("q", [1, 25, 50, 75, 90, 95, 100])
def test_quant_tables_are_libjpegs(q):
    from nerf.jpeg import quant_tables
    order = _pil_order()
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG", quality=q)
    theirs = Image.open(io.BytesIO(buf.getvalue())).quantization
    ours = quant_tables(q)
    assert ours[0].dtype == np.uint16 and ours[0].shape == (64,)
    for i in range(2):
        assert _natural(theirs[i], order) == ours[i].tolist(), (q, i)
    with pytest.raises(ValueError):
        quant_tables(0)
    with pytest.raises(ValueError):
        quant_tables(101)


def _dht(data):
    """{Tc << 4 | Th: (BITS, HUFFVAL)} of a JPEG file's DHT segments."""
    out, i = {}, 2
    while i < len(data):
        marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if marker == 0xC4:
            seg, j = data[i + 4:i + 2 + length], 0
            while j < len(seg):
                bits = list(seg[j + 1:j + 17])
                out[seg[j]] = (bits, list(seg[j + 17:j + 17 + sum(bits)]))
                j += 17 + sum(bits)
        if marker == 0xDA:
            break
        i += 2 + length
    return out


def test_huffman_tables_agree_everywhere():
    """nerf/jpeg.py, csrc/jpeg_tables.h, the helper and libjpeg's defaults (which
    are Annex K.3) hold the same BITS / HUFFVAL; the zigzag sequences agree."""
    from nerf import jpeg
    ours = {0x00: jpeg.DC_LUMA, 0x10: jpeg.AC_LUMA, 0x01: jpeg.DC_CHROMA, 0x11: jpeg.AC_CHROMA}
    helper = {0x00: jh._K3, 0x10: jh._K5, 0x01: jh._K4, 0x11: jh._K6}
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG", quality=90)
    pil = _dht(buf.getvalue())
    src = open(os.path.join(ROOT, "torch-ngp_amd", "csrc", "jpeg_tables.h")).read()
    arrays = {name: [int(v, 0) for v in body.replace("\n", " ").split(",") if v.strip()]
              for name, body in re.findall(r"(kJpeg\w+)\[\d+\] = \{([^}]*)\}", src)}
    header = {0x00: ("DcLuma",), 0x10: ("AcLuma",), 0x01: ("DcChroma",), 0x11: ("AcChroma",)}
    assert sorted(pil) == sorted(ours)
    for key, (bits, vals) in ours.items():
        assert (list(bits), list(vals)) == (list(helper[key][0]), list(helper[key][1])) == tuple(pil[key]), hex(key)
        stem = "kJpeg" + header[key][0]
        assert arrays[stem + "Bits"] == list(bits) and arrays[stem + "Vals"] == list(vals), stem
    assert arrays["kJpegZigzag"] == list(jpeg.ZIGZAG) == jh.ZIGZAG
    assert sorted(jh.ZIGZAG) == list(range(64))
    # the header a file starts with carries them: PIL reads the same tables back out of it
    assert _dht(jpeg.header(8, 8, 3, jpeg.quant_tables(90))) == pil
    assert sorted(_dht(jpeg.header(8, 8, 1, jpeg.quant_tables(90)))) == [0x00, 0x10]


def _encode_ref(image, quality, symbols=None):
    from nerf import jpeg
    H, W = image.shape[:2]
    comps = 1 if image.ndim == 2 else 3
    tables = jpeg.quant_tables(quality)
    coefs, quot = jh.ref_coefficients(image, tables)
    scan = jh.ref_scan(coefs, H, W, comps, symbols)
    return jpeg.header(H, W, comps, tables) + scan + jpeg.EOI, coefs, scan, tables


@pytest.mark.parametrize("comps", [1, 3])
@pytest.mark.parametrize("shape", jh.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_files_load_in_pil(shape, comps, capsys):
    import _ngp_native as nat
    H, W = shape
    worst = 0
    for kind, quality in jh.cases(H, W):
        image = jh.make_image(kind, H, W, comps)
        symbols = []
        data, coefs, scan, tables = _encode_ref(image, quality, symbols)
        im = jh.pil_decode(data)
        assert im.size == (W, H) and im.mode == ("L" if comps == 1 else "RGB"), (kind, quality)
        diff = int(np.abs(np.asarray(im).astype(np.int32) -
                          jh.ref_decode(coefs, H, W, comps, tables).astype(np.int32)).max())
        worst = max(worst, diff)
        assert diff <= jh.DECODE_BOUND[comps], (kind, quality, diff)
        if os.path.exists(nat.LIB_PATH):
            assert len(scan) <= nat.lib().ngp_jpeg_scan_capacity(H, W, comps)
        # what each image is there for
        blocks = coefs.reshape(-1, comps, 64)
        if kind.startswith("flat"):
            assert not blocks[:, :, 1:].any() and 0x00 in symbols  # EOB-only blocks
            assert symbols.count(0) >= blocks.shape[0] * comps  # ... and DC differences of category 0 after the first
        if kind == "checker" and quality == 100:
            assert any(s & 15 == 10 for s in symbols)  # the largest AC category
            assert 511 < np.abs(blocks[:, 0, 1:]).max() <= 1023  # ... and inside the clamp
        if kind == "cos77":
            assert blocks[:, 0, 63].all() and not blocks[:, 0, :63].any()  # only coefficient 63
            assert symbols.count(0xF0) >= 3 * blocks.shape[0]  # three ZRL before it
        if kind == "noise" and quality == 100:
            assert b"\xff\x00" in scan  # a stuffed byte
        if (H, W) == (80, 8):
            marks = re.findall(rb"\xff[\xd0-\xd7]", scan)
            assert marks == [bytes([0xFF, 0xD0 + (i & 7)]) for i in range(9)]  # ... D7, then D0 again
    with capsys.disabled():
        print(f"\n  {H}x{W}x{comps}: max |PIL decode - float64 decode| = {worst} (bound {jh.DECODE_BOUND[comps]})")


def test_psnr_gap_of_the_reference_encoder(capsys):
    """PIL's own encoding with the same tables against the reference encoder's
    file, both decoded by PIL: the gap the GPU test's margin is built on."""
    order = _pil_order()
    worst, where = -1e9, None
    for comps in (1, 3):
        for H, W, kind, quality in jh.PSNR_CASES:
            image = jh.make_image(kind, H, W, comps)
            data, _, _, tables = _encode_ref(image, quality)
            theirs = jh.pil_encode(image, tables)
            got = Image.open(io.BytesIO(theirs)).quantization
            for i in range(1 if comps == 1 else 2):  # PIL did use our tables
                assert _natural(got[i], order) == tables[i].tolist()
            a, b = jh.psnr(np.asarray(jh.pil_decode(theirs)), image), jh.psnr(np.asarray(jh.pil_decode(data)), image)
            gap = 0.0 if a == b else a - b
            if gap > worst:
                worst, where = gap, (H, W, comps, kind, quality, round(a, 3), round(b, 3))
    with capsys.disabled():
        print(f"\n  largest PSNR gap, PIL's encoder minus the reference encoder: {worst:.4f} dB at {where}")
    assert worst <= jh.PSNR_GAP_MEASURED


def test_header_layout():
    from nerf import jpeg
    tables = jpeg.quant_tables(75)
    h = jpeg.header(37, 53, 3, tables)
    assert h[:4] == b"\xff\xd8\xff\xe0" and h[6:11] == b"JFIF\x00"
    i, seen = 2, []
    while i < len(h):
        assert h[i] == 0xFF
        length = (h[i + 2] << 8) | h[i + 3]
        seen.append((h[i + 1], h[i + 4:i + 2 + length]))
        i += 2 + length
    assert i == len(h)
    assert [m for m, _ in seen] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    dqt = seen[1][1]
    assert dqt[0] == 0 and list(dqt[1:]) == [int(tables[0][n]) for n in jh.ZIGZAG]  # zigzag order
    assert seen[3][1] == bytes([8, 0, 37, 0, 53, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert seen[8][1] == bytes([0, 7])  # DRI: ceil(53 / 8) MCUs
    assert seen[9][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    g = jpeg.header(8, 8, 1, tables)
    assert g.count(b"\xff\xdb") == 1 and g.count(b"\xff\xc4") == 2
    for bad in ((0, 8, 3), (8, 70000, 3), (8, 8, 2)):
        with pytest.raises(ValueError):
            jpeg.header(*bad, tables)


def test_entry_argument_errors_need_no_gpu():
    import _ngp_native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libngp_hip.so not built")
    lib = nat.lib()
    assert lib.ngp_jpeg_scan_capacity(8, 8, 2) == 0 and lib.ngp_jpeg_workspace_elems(0, 8, 3) == 0
    assert lib.ngp_jpeg_scan_capacity(8, 70000, 3) == 0
    # n * (2 * (216 * B + 1) + 2)
    assert lib.ngp_jpeg_scan_capacity(8, 8, 1) == 2 * 217 + 2
    assert lib.ngp_jpeg_scan_capacity(17, 9, 3) == 3 * (2 * (216 * 6 + 1) + 2)
    assert lib.ngp_jpeg_scan_capacity(800, 800, 3) == 100 * (2 * (216 * 300 + 1) + 2)
    assert lib.ngp_jpeg_workspace_elems(8, 8, 1) >= 64 + (4 + 2 * 217) // 2
    q = (ctypes.c_uint16 * 64)(*([16] * 64))
    cap = lib.ngp_jpeg_scan_capacity(8, 8, 3)
    one = ctypes.c_void_p(16)  # non-null, aligned, never dereferenced: every check below fails first

    def call(pixels=one, H=8, W=8, comps=3, ql=q, qc=q, ws=one, out=one, capacity=cap, out_len=one):
        return lib.ngp_jpeg_encode(pixels, H, W, comps, ql, qc, ws, out, capacity, out_len, None)

    for kwargs, text in (({"pixels": None}, b"null"), ({"ql": None}, b"null"), ({"qc": None}, b"null"),
                         ({"ws": None}, b"null"), ({"out": None}, b"null"), ({"out_len": None}, b"null"),
                         ({"comps": 2}, b"components"), ({"comps": 0}, b"components"), ({"H": 0}, b"H and W"),
                         ({"W": 0}, b"H and W"), ({"W": 65536}, b"H and W"), ({"capacity": cap - 1}, b"capacity"),
                         ({"ws": ctypes.c_void_p(8)}, b"aligned")):
        assert call(**kwargs) == -1, kwargs
        assert text in lib.ngp_last_error(), (kwargs, lib.ngp_last_error())
    for bad in (0, 256):
        t = (ctypes.c_uint16 * 64)(*([16] * 63 + [bad]))
        assert call(ql=t) == -1 and b"quantiser 63" in lib.ngp_last_error()
        assert call(qc=t) == -1 and b"quantiser" in lib.ngp_last_error()
    # one component needs no chrominance table: the call gets as far as the capacity check
    assert call(comps=1, qc=None, capacity=0) == -1 and b"capacity" in lib.ngp_last_error()
