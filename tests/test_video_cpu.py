"""CPU: the Motion-JPEG AVI container (nerf/video.py): a written file reads
back byte for byte, its header fields sit where AVI 1.0 puts them, idx1 agrees
with movi, and the 2 GB guard raises before a file would outgrow the format."""
import struct

import numpy as np
import pytest

import jpeg_helpers as jh


def _frames():
    """Three real JPEG files of 24 x 16 (reference encoder), and odd / even lengths among them."""
    from nerf import jpeg
    out = []
    for kind in ("noise", "hramp", "checker"):
        image = jh.make_image(kind, 16, 24, 3)
        tables = jpeg.quant_tables(90)
        coefs, _ = jh.ref_coefficients(image, tables)
        out.append(jpeg.header(16, 24, 3, tables) + jh.ref_scan(coefs, 16, 24, 3) + jpeg.EOI)
    if all(len(f) % 2 == len(out[0]) % 2 for f in out):
        out[1] += b"\x00"  # (bytes after EOI are ignored by decoders) make one length differ in parity
    assert {len(f) % 2 for f in out} == {0, 1}
    return out


def test_round_trip_and_header_offsets(tmp_path):
    from nerf.video import OFFSETS, AviWriter, read_avi
    frames = _frames()
    path = str(tmp_path / "a.avi")
    w = AviWriter(path, 24, 16, 25)
    for f in frames:
        w.add(f)
    w.close()
    w.close()  # idempotent
    info, got = read_avi(path)
    assert got == frames
    assert (info["width"], info["height"], info["fps"], info["frames"]) == (24, 16, 25.0, 3)
    assert (info["handler"], info["compression"], info["type"], info["bit_count"]) == ("MJPG", "MJPG", "vids", 24)
    data = open(path, "rb").read()
    u32 = lambda name: struct.unpack_from("<I", data, OFFSETS[name])[0]  # noqa: E731
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and data[12:16] == b"LIST" and data[20:28] == b"hdrlavih"
    assert u32("riff_size") == len(data) - 8
    assert u32("usec_per_frame") == 40000 and u32("total_frames") == 3 and u32("streams") == 1
    assert u32("flags") & 0x10  # AVIF_HASINDEX
    assert u32("width") == 24 and u32("height") == 16
    assert data[100:104] == b"strh" and data[OFFSETS["fcc_type"]:OFFSETS["fcc_type"] + 8] == b"vidsMJPG"
    assert u32("scale") == 1 and u32("rate") == 25 and u32("length") == 3
    assert u32("suggested_buffer") == max(len(f) for f in frames)
    assert data[164:168] == b"strf" and u32("bi_width") == 24 and u32("bi_height") == 16
    assert struct.unpack_from("<H", data, OFFSETS["bi_bit_count"])[0] == 24
    assert data[OFFSETS["bi_compression"]:OFFSETS["bi_compression"] + 4] == b"MJPG"
    assert data[212:216] == b"LIST" and data[220:228] == b"movi00dc"
    # movi: chunks padded to even length; idx1 right after it
    movi_end = 220 + u32("movi_size")
    assert movi_end % 2 == 0 and data[movi_end:movi_end + 4] == b"idx1"
    assert struct.unpack_from("<I", data, movi_end + 4)[0] == 16 * 3 and movi_end + 8 + 48 == len(data)
    at = 224
    for k, f in enumerate(frames):
        assert data[at:at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == len(f)
        assert struct.unpack_from("<4sIII", data, movi_end + 8 + 16 * k) == (b"00dc", 0x10, at - 220, len(f))
        at += 8 + len(f) + (len(f) & 1)
    assert at == movi_end
    # every frame is a JPEG PIL opens
    for f in got:
        assert jh.pil_decode(f).size == (24, 16)


def test_grey_frames_and_context_manager(tmp_path):
    from nerf import jpeg
    from nerf.video import AviWriter, read_avi
    image = jh.make_image("vramp", 9, 17, 1)
    tables = jpeg.quant_tables(50)
    coefs, _ = jh.ref_coefficients(image, tables)
    f = jpeg.header(9, 17, 1, tables) + jh.ref_scan(coefs, 9, 17, 1) + jpeg.EOI
    path = str(tmp_path / "g.avi")
    with AviWriter(path, 17, 9, 30) as w:
        w.add(f)
    info, got = read_avi(path)
    assert got == [f] and info["fps"] == 30 and info["frames"] == 1
    im = jh.pil_decode(got[0])
    assert im.mode == "L" and np.abs(np.asarray(im).astype(int) - image.astype(int)).max() < 40
    with pytest.raises(ValueError):
        w.add(f)  # closed


def test_an_empty_file_is_still_a_file(tmp_path):
    from nerf.video import AviWriter, read_avi
    path = str(tmp_path / "e.avi")
    AviWriter(path, 8, 8, 25).close()
    info, got = read_avi(path)
    assert got == [] and info["frames"] == 0


def test_two_gigabyte_guard(tmp_path):
    from nerf import video
    path = str(tmp_path / "big.avi")
    w = video.AviWriter(path, 8, 8, 25)
    frame = b"\xff\xd8" + b"\x00" * 97 + b"\xff\xd9"  # 101 bytes -> a chunk of 8 + 101 + 1
    w.add(frame)
    # as if just under 2 GB had been written: this frame, its idx1 entry and idx1's header must still fit
    room = 110 + 8 + 16 * 2
    w._size = video.MAX_BYTES - room
    w.add(frame)  # ends exactly at 2^31 - 1
    assert w._size == video.MAX_BYTES - room + 110
    w._size = video.MAX_BYTES - (110 + 8 + 16 * 3) + 1  # one byte too many for a third frame
    with pytest.raises(ValueError, match=r"2\^31 - 1"):
        w.add(frame)
    assert len(w._index) == 2
    w._f.close()  # (the mocked size would make close() write sizes that are not the file's)
    w._f = None


def test_read_avi_rejects_a_broken_index(tmp_path):
    from nerf.video import AviWriter, read_avi
    path = str(tmp_path / "a.avi")
    with AviWriter(path, 24, 16, 25) as w:
        for f in _frames():
            w.add(f)
    data = bytearray(open(path, "rb").read())
    data[-4] ^= 1  # the last idx1 entry's size
    bad = str(tmp_path / "b.avi")
    open(bad, "wb").write(bytes(data))
    with pytest.raises(ValueError, match="idx1"):
        read_avi(bad)
    with pytest.raises(ValueError, match="RIFF"):
        open(bad, "wb").write(b"not an avi file")
        read_avi(bad)
    with pytest.raises(ValueError):
        AviWriter(str(tmp_path / "c.avi"), 8, 8, 0)
