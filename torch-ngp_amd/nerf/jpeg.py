"""Baseline JPEG files of uint8 frames that stay on the device (csrc/jpeg.hip,
DESIGN.md §19): the library writes the entropy-coded scan, this module the
header segments and EOI around it.

The file: SOI, APP0 (JFIF 1.01), DQT, SOF0 (8 bit, 3 components sampled 1 x 1
or 1 component), DHT (the typical tables of T.81 Annex K.3), DRI (one MCU row),
SOS, the scan, EOI. The quantisation tables are Annex K.1 / K.2 scaled by the
libjpeg quality rule, so `quality` means what it means to every other encoder.
"""
import ctypes
import struct

import numpy as np
import torch

import _ngp_native as nat

# T.81 Annex K.1 (luminance) and K.2 (chrominance), natural (row-major) order
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
           14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
             47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# T.81 Figure A.6: ZIGZAG[k] is the natural index of the k-th coefficient of the zigzag sequence
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
          14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
          46, 53, 60, 61, 54, 47, 55, 62, 63)

# T.81 Annex K.3, Tables K.3 to K.6: (BITS, HUFFVAL), the numbers of csrc/jpeg_tables.h
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), tuple(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))

EOI = b"\xff\xd9"


def quant_tables(quality):
    """(luma, chroma), uint16 [64] each in natural order: K.1 / K.2 scaled by
    the libjpeg rule, s = 5000 // q below 50, else 200 - 2 q; each entry
    clip((base * s + 50) // 100, 1, 255)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quant_tables: quality must be in 1..100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(base, dtype=np.int64) * s + 50) // 100, 1, 255).astype(np.uint16)
                 for base in (K1_LUMA, K2_CHROMA))


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def header(H, W, components, tables):
    """The bytes before the scan: SOI, APP0 / JFIF, DQT (zigzag order), SOF0,
    DHT (all four tables, or the two luminance ones for 1 component), DRI (one
    MCU row), SOS. tables: (luma, chroma) as quant_tables gives them."""
    if components not in (1, 3):
        raise ValueError(f"header: components must be 1 or 3, got {components}")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"header: H and W must be in 1..65535, got {H} x {W}")
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for tq in range(1 if components == 1 else 2):
        t = np.asarray(tables[tq]).reshape(64)
        if t.min() < 1 or t.max() > 255:
            raise ValueError("header: baseline quantisers are 1..255")
        out.append(_segment(0xDB, bytes([tq]) + bytes(int(t[n]) for n in ZIGZAG)))
    sof = struct.pack(">BHHB", 8, H, W, components)
    for c in range(components):
        sof += bytes([c + 1, 0x11, 0 if c == 0 else 1])
    out.append(_segment(0xC0, sof))
    huff = [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([(0x01, DC_CHROMA), (0x11, AC_CHROMA)] if components == 3 else [])
    for tc_th, (bits, vals) in huff:
        out.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack(">H", (W + 7) // 8)))
    sos = bytes([components])
    for c in range(components):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    out.append(_segment(0xDA, sos + bytes([0, 63, 0])))
    return b"".join(out)


class JpegEncoder:
    """Encoder of [H, W, 3] (RGB) or [H, W] (grey) uint8 device tensors of one
    size. It owns the library's workspace, the scan buffer, the scan length and
    two pinned host buffers.

    encode(t) -> the bytes of a complete JPEG file.

    submit(t) / result(): the split form. submit enqueues the three launches
    and the copy of the length, waits for the length (the one host wait of the
    image) and enqueues the copy of exactly that many scan bytes into one of
    the two pinned buffers, without waiting for it. result() returns the oldest
    submitted image's file; it waits only if nothing submitted later has
    already proven the copy done (the stream runs in order), so in a loop that
    submits frame i + 1 before it takes frame i's result, frame i's bytes land
    while frame i + 1 renders and every image costs one wait. At most two
    images are in flight."""

    def __init__(self, H, W, components, quality=90, device="cuda"):
        self.H, self.W, self.components = int(H), int(W), int(components)
        if self.components not in (1, 3):
            raise ValueError(f"JpegEncoder: components must be 1 or 3, got {components}")
        self.dev = torch.device(device)
        self.tables = quant_tables(quality)
        self.header = header(self.H, self.W, self.components, self.tables)
        lib = nat.lib()
        self.capacity = int(lib.ngp_jpeg_scan_capacity(self.H, self.W, self.components))
        elems = int(lib.ngp_jpeg_workspace_elems(self.H, self.W, self.components))
        if self.capacity == 0 or elems == 0:
            raise ValueError(f"JpegEncoder: H and W must be in 1..65535, got {H} x {W}")
        self.blocks = ((self.H + 7) // 8) * ((self.W + 7) // 8) * self.components
        self.workspace = torch.zeros(elems, dtype=torch.int16, device=self.dev)
        self.scan = torch.zeros(self.capacity, dtype=torch.uint8, device=self.dev)
        self.scan_len = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._q = [(ctypes.c_uint16 * 64)(*[int(v) for v in t]) for t in self.tables]
        self._host = None   # two (pinned scan, pinned length, copy event) slots
        self._pending = []  # [slot, length, sequence number] of submitted images, oldest first
        self._seq = 0       # images submitted
        self._proven = 0    # every copy of an image with a sequence number below this is done

    def coefficients(self):
        """The quantised coefficients of the last image, int16 [blocks, 64] in
        zigzag order, blocks in MCU order (a view of the workspace)."""
        return self.workspace[:self.blocks * 64].view(self.blocks, 64)

    def _check(self, t):
        shape = (self.H, self.W, 3) if self.components == 3 else (self.H, self.W)
        nat.check_tensor(t, "JpegEncoder: the image", (torch.uint8,), "uint8")
        if tuple(t.shape) != shape:
            raise ValueError(f"JpegEncoder: the image must be {list(shape)}, got {list(t.shape)}")

    def launch(self, t):
        """The three launches on the current stream; nothing is waited for."""
        self._check(t)
        P = nat.ptr
        nat.check(nat.lib().ngp_jpeg_encode(P(t), self.H, self.W, self.components, self._q[0], self._q[1],
                                            P(self.workspace), P(self.scan), self.capacity, P(self.scan_len),
                                            nat.stream_of(self.scan)), "jpeg_encode")

    def submit(self, t):
        if len(self._pending) == 2:
            raise RuntimeError("JpegEncoder: two images are in flight; take a result() first")
        if self._host is None:
            self._host = [(torch.empty(self.capacity, dtype=torch.uint8).pin_memory(),
                           torch.empty(1, dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(2)]
        slot = self._seq & 1
        buf, length, event = self._host[slot]
        self.launch(t)
        length.copy_(self.scan_len, non_blocking=True)
        event.record()
        event.synchronize()  # the image's one wait; everything enqueued before it is done too
        self._proven = self._seq
        n = int(length.item()) & 0xFFFFFFFF  # (a uint32 on the device)
        buf[:n].copy_(self.scan[:n], non_blocking=True)
        event.record()
        self._pending.append((slot, n, self._seq))
        self._seq += 1

    def result(self):
        if not self._pending:
            raise RuntimeError("JpegEncoder: result() without a submit()")
        slot, n, seq = self._pending.pop(0)
        buf, _, event = self._host[slot]
        if seq >= self._proven:  # no later submit has waited past this image's copy
            event.synchronize()
        return b"".join((self.header, buf[:n].numpy().tobytes(), EOI))

    def encode(self, t):
        if self._pending:
            raise RuntimeError("JpegEncoder: encode() with submitted images in flight")
        self.submit(t)
        return self.result()
