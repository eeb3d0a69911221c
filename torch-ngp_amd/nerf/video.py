"""Motion-JPEG in an AVI 1.0 file, host only: the container of the test render's
videos (nerf.frames.write_video). Every frame is a complete
baseline JPEG file (nerf/jpeg.py) in a `00dc` chunk.

    RIFF 'AVI '
      LIST 'hdrl'
        'avih'  MainAVIHeader (56 bytes)
        LIST 'strl'
          'strh'  AVIStreamHeader (56 bytes): 'vids' / 'MJPG', rate fps, scale 1
          'strf'  BITMAPINFOHEADER (40 bytes): biCompression 'MJPG', 24 bit
      LIST 'movi'
        '00dc' <size> <jpeg> [pad to even]   one per frame
      'idx1'  16 bytes per frame: '00dc', AVIIF_KEYFRAME, offset from 'movi', size

There is no OpenDML extension, so a file ends below 2^31 - 1 bytes.
"""
import os
import struct

MAX_BYTES = 2 ** 31 - 1
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
_MOVI_LIST = 212   # offset of the 'LIST' of movi; its size at 216, 'movi' at 220, the first chunk at 224
# byte offsets of the fields close() patches, and of those a reader may want to look at
OFFSETS = {"riff_size": 4, "usec_per_frame": 32, "max_bytes_per_sec": 36, "flags": 44, "total_frames": 48,
           "streams": 56, "suggested_buffer": 60, "width": 64, "height": 68, "fcc_type": 108, "fcc_handler": 112,
           "scale": 128, "rate": 132, "length": 140, "stream_suggested_buffer": 144, "bi_width": 176,
           "bi_height": 180, "bi_bit_count": 186, "bi_compression": 188, "movi_size": 216}


class AviWriter:
    """AviWriter(path, W, H, fps); add(jpeg_bytes) per frame; close() writes
    idx1 and patches the sizes and the frame count. Usable as a context
    manager."""

    def __init__(self, path, W, H, fps):
        if int(fps) != fps or fps < 1:
            raise ValueError(f"AviWriter: fps must be a positive integer (rate fps, scale 1), got {fps}")
        if not (1 <= W <= 65535 and 1 <= H <= 65535):
            raise ValueError(f"AviWriter: W and H must be in 1..65535, got {W} x {H}")
        self.path, self.W, self.H, self.fps = path, int(W), int(H), int(fps)
        self._index = []  # (offset from 'movi', size) per frame
        self._largest = 0
        self._f = open(path, "wb")
        self._f.write(self._headers(0, 0, 0))
        self._size = self._f.tell()  # bytes written so far
        assert self._size == _MOVI_LIST + 12

    def _headers(self, frames, movi_size, riff_size):
        W, H, fps = self.W, self.H, self.fps
        avih = struct.pack("<14I", 1000000 // fps, self._largest * fps, 0, AVIF_HASINDEX, frames, 0, 1,
                           self._largest, W, H, 0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4h", 0, 0, 0, 0, 1, fps, 0, frames, self._largest, 0xFFFFFFFF,
                                         0, 0, 0, W, H)
        strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        return (b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
                b"LIST" + struct.pack("<I", movi_size) + b"movi")

    def add(self, jpeg):
        if self._f is None:
            raise ValueError("AviWriter: add() after close()")
        n = len(jpeg)
        chunk = 8 + n + (n & 1)
        final = self._size + chunk + 8 + 16 * (len(self._index) + 1)  # the file if it were closed after this frame
        if final > MAX_BYTES:
            raise ValueError(f"AviWriter: {self.path} would reach {final} bytes with this frame; AVI 1.0 (no OpenDML "
                             f"extension) ends at 2^31 - 1 = {MAX_BYTES} bytes")
        self._index.append((self._size - (_MOVI_LIST + 8), n))
        self._f.write(b"00dc" + struct.pack("<I", n) + jpeg + (b"\x00" if n & 1 else b""))
        self._size += chunk
        self._largest = max(self._largest, n)

    def close(self):
        if self._f is None:
            return
        f, n = self._f, len(self._index)
        idx = b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, off, size) for off, size in self._index)
        f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        total = self._size + 8 + len(idx)
        f.seek(0)
        f.write(self._headers(n, self._size - (_MOVI_LIST + 8), total - 8))
        f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _chunks(data, start, end):
    """(fourcc, payload offset, size) of the chunks in data[start:end]."""
    at = start
    while at + 8 <= end:
        fourcc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        if at + 8 + size > end:
            raise ValueError(f"read_avi: chunk {fourcc!r} at {at} runs past its parent ({size} bytes)")
        yield fourcc, at + 8, size
        at += 8 + size + (size & 1)


def read_avi(path):
    """-> (info, frames): info = {width, height, fps, scale, rate, frames,
    handler, compression, bit_count, usec_per_frame}, frames = the bytes of
    every `00dc` chunk in order. The chunk tree is walked, not assumed, and
    idx1 must list exactly movi's chunks (offset from 'movi', size, keyframe):
    ValueError otherwise."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"read_avi: {path} is not a RIFF AVI file")
    riff_size = struct.unpack_from("<I", data, 4)[0]
    if riff_size + 8 != len(data):
        raise ValueError(f"read_avi: RIFF size {riff_size} + 8 is not the file's {len(data)} bytes")
    info, frames, movi, index = {}, [], [], None
    for fourcc, at, size in _chunks(data, 12, len(data)):
        if fourcc == b"LIST" and data[at:at + 4] == b"hdrl":
            for cc, a, s in _chunks(data, at + 4, at + size):
                if cc == b"avih":
                    v = struct.unpack_from("<14I", data, a)
                    info.update(usec_per_frame=v[0], flags=v[3], frames=v[4], streams=v[6], width=v[8], height=v[9])
                elif cc == b"LIST" and data[a:a + 4] == b"strl":
                    for c2, a2, s2 in _chunks(data, a + 4, a + s):
                        if c2 == b"strh":
                            info.update(type=data[a2:a2 + 4].decode("latin1"),
                                        handler=data[a2 + 4:a2 + 8].decode("latin1"))
                            scale, rate, _, length = struct.unpack_from("<4I", data, a2 + 20)
                            info.update(scale=scale, rate=rate, fps=rate / scale, stream_length=length)
                        elif c2 == b"strf":
                            bi = struct.unpack_from("<IiiHH4sI", data, a2)
                            info.update(bi_width=bi[1], bi_height=bi[2], bit_count=bi[4],
                                        compression=bi[5].decode("latin1"))
        elif fourcc == b"LIST" and data[at:at + 4] == b"movi":
            for cc, a, s in _chunks(data, at + 4, at + size):
                if cc == b"00dc":
                    frames.append(data[a:a + s])
                    movi.append((a - 8 - at, s))
        elif fourcc == b"idx1":
            index = [struct.unpack_from("<4sIII", data, at + 16 * k) for k in range(size // 16)]
    if "frames" not in info or "rate" not in info or "compression" not in info:
        raise ValueError(f"read_avi: {path} lacks avih, strh or strf")
    if index is None:
        raise ValueError(f"read_avi: {path} has no idx1")
    if [(cc, off, s) for cc, _, off, s in index] != [(b"00dc", off, s) for off, s in movi]:
        raise ValueError(f"read_avi: idx1 of {path} does not list movi's chunks")
    if any(not flags & AVIIF_KEYFRAME for _, flags, _, _ in index):
        raise ValueError(f"read_avi: idx1 of {path} has a frame that is not a key frame")
    if info["frames"] != len(frames) or info["stream_length"] != len(frames):
        raise ValueError(f"read_avi: the headers of {path} count {info['frames']} / {info['stream_length']} frames, "
                         f"movi holds {len(frames)}")
    return info, frames
