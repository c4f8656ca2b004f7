"""Baseline JPEG encoder in numpy: the restatement csrc/jpeg.hip must equal byte for byte (and Pillow / libjpeg with it).

Written from ITU-T T.81 (tables of Annex K, marker syntax of Annex B) and libjpeg's documented integer arithmetic:

* colour: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
  Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16;
* 4:2:0 chroma: the frame is extended to whole 16-pixel MCU columns by replicating its last column, and by one row when its height is
  odd; each 2 x 2 box is (sum + bias) >> 2 with bias 1, 2, 1, 2, ... along a row; the DOWNSAMPLED planes are then extended to whole
  MCU rows by replicating their last row (so with an even height the rows below the frame repeat the last 2-row average);
* forward DCT: level shift by 128, the "islow" 13-bit integer DCT (rows with PASS1_BITS = 2 kept, then columns), outputs scaled by 8;
* quantisation: round-half-away-from-zero division by 8 q[i], q = Annex K table * IJG quality scale, clamped to 1..255;
* luminance blocks that only fill the last MCU column / row are dummy blocks: AC zero, DC of the preceding block of the MCU;
* Huffman coding with the Annex K.3-K.6 tables, MCU order Y00 Y01 Y10 Y11 Cb Cr, 1-padding, 0xFF00 stuffing;
* markers: SOI, APP0 (JFIF 1.01, no units, 1 x 1), DQT per table, SOF0, DHT per table, SOS, scan, EOI.

The transform is vectorised; the bit writer is a plain Python loop over blocks.
"""
from __future__ import annotations

import struct
from typing import List, Tuple

import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99])

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa]


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """(luminance, chrominance) in natural order: Annex K scaled the IJG way, 1..255"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be in 1..100, got {quality}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255).astype(np.int64) for t in (LUMA_Q, CHROMA_Q))


def huff_codes(bits, vals):
    """symbol -> (code, length), canonical codes of Annex C"""
    out = {}
    code = 0
    k = 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _fdct_1d(d, first_pass: bool):
    """libjpeg's jfdctint over the last axis (int64 in, int64 out)"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first_pass else 13 + 2

    def ds(x, s):
        return (x + (1 << (s - 1))) >> s

    o = [None] * 8
    if first_pass:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = ds(t10 + t11, 2), ds(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = ds(z1 + t13 * 6270, n)
    o[6] = ds(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, n), ds(t5 + z2 + z4, n), ds(t6 + z2 + z3, n), ds(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _blocks_quantised(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """plane [8 by][8 bx] uint8 -> [by][bx][64] quantised coefficients in zig-zag order"""
    h, w = plane.shape
    b = plane.astype(np.int64).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128        # [by][bx][row][col]
    b = _fdct_1d(b, True)                                                                       # rows
    b = _fdct_1d(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)                          # columns
    c = b.reshape(h // 8, w // 8, 64)
    d = q.reshape(1, 1, 64) * 8
    a = (np.abs(c) + (d >> 1)) // d
    return (np.sign(c) * a)[:, :, ZIGZAG]


def _hwc(frame) -> np.ndarray:
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise ValueError(f"frames must be uint8, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"frames must be HxW or HxWxC with C = 1 or 3, got shape {a.shape}")
    return a


def coefficients(frame, quality: int) -> np.ndarray:
    """quantised zig-zag blocks in scan order, int16 [blocks][64]: C = 1 raster order of the 8 x 8 blocks; C = 3 (BGR) per MCU
    Y00 Y01 Y10 Y11 Cb Cr"""
    a = _hwc(frame)
    H, W, C = a.shape
    ql, qc = quant_tables(quality)
    if C == 1:
        g = np.pad(a[:, :, 0], ((0, -H % 8), (0, -W % 8)), mode="edge")
        return _blocks_quantised(g, ql).reshape(-1, 64).astype(np.int16)
    p = np.pad(a, ((0, H % 2), (0, -W % 16), (0, 0)), mode="edge").astype(np.int64)      # rows: to a whole 2-row group only
    B, G, R = p[:, :, 0], p[:, :, 1], p[:, :, 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    pw = Y.shape[1]
    bias = np.tile(np.array([1, 2]), pw // 4)[None, :]

    def down(x):
        return (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + bias) >> 2

    my, mx = (H + 15) // 16, pw // 16

    def rows_to(x, n):                                                 # the DOWNSAMPLED planes are extended downwards by their last row
        return np.pad(x, ((0, n - x.shape[0]), (0, 0)), mode="edge").astype(np.uint8)

    yb = _blocks_quantised(rows_to(Y, 16 * my), ql)                    # [2 my][2 mx][64]
    cb = _blocks_quantised(rows_to(down(Cb), 8 * my), qc)              # [my][mx][64]
    cr = _blocks_quantised(rows_to(down(Cr), 8 * my), qc)
    hb, wb = (H + 7) // 8, (W + 7) // 8                                # real luminance blocks
    out = np.zeros((my, mx, 6, 64), np.int64)
    for k in range(4):
        out[:, :, k] = yb[k >> 1::2, k & 1::2]
    out[:, :, 4], out[:, :, 5] = cb, cr
    if wb < 2 * mx:                                                    # dummy blocks at the right edge: DC of the block to the left
        for k in (1, 3):
            out[:, mx - 1, k, 1:] = 0
            out[:, mx - 1, k, 0] = out[:, mx - 1, k - 1, 0]
    if hb < 2 * my:                                                    # a dummy block row at the bottom: DC of the MCU's block 1
        for k in (2, 3):
            out[my - 1, :, k, 1:] = 0
            out[my - 1, :, k, 0] = out[my - 1, :, 1, 0]
    return out.reshape(-1, 64).astype(np.int16)


def _marker(tag: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, tag, len(payload) + 2) + payload


def headers(H: int, W: int, C: int, quality: int) -> bytes:
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _marker(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _marker(0xDB, bytes([0]) + bytes(int(v) for v in ql[ZIGZAG]))
    if C == 3:
        out += _marker(0xDB, bytes([1]) + bytes(int(v) for v in qc[ZIGZAG]))
    comps = [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)] if C == 3 else [(1, 0x11, 0)]
    out += _marker(0xC0, struct.pack(">BHHB", 8, H, W, len(comps)) + b"".join(bytes(c) for c in comps))
    out += _marker(0xC4, bytes([0x00] + DC_LUMA_BITS + DC_VALS))
    out += _marker(0xC4, bytes([0x10] + AC_LUMA_BITS + AC_LUMA_VALS))
    if C == 3:
        out += _marker(0xC4, bytes([0x01] + DC_CHROMA_BITS + DC_VALS))
        out += _marker(0xC4, bytes([0x11] + AC_CHROMA_BITS + AC_CHROMA_VALS))
    sel = [(1, 0x00), (2, 0x11), (3, 0x11)] if C == 3 else [(1, 0x00)]
    out += _marker(0xDA, bytes([len(sel)]) + b"".join(bytes(s) for s in sel) + b"\x00\x3f\x00")
    return out


_DC = [huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS)]
_AC = [huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS)]


def scan_bytes(coefs: np.ndarray, C: int) -> bytes:
    """entropy-coded segment of the blocks in scan order (stuffed, padded with 1-bits)"""
    nb = coefs.shape[0]
    rows = coefs.tolist()
    out = bytearray()
    acc = 0
    nacc = 0
    pred = [0, 0, 0]
    for i in range(nb):
        k = i % 6 if C == 3 else 0
        comp = 0 if k < 4 else k - 3
        dc, ac = _DC[comp > 0], _AC[comp > 0]
        blk = rows[i]
        diff = blk[0] - pred[comp]
        pred[comp] = blk[0]
        s = abs(diff).bit_length()
        code, ln = dc[s]
        acc = (acc << ln) | code
        nacc += ln
        if s:
            acc = (acc << s) | ((diff if diff >= 0 else diff - 1) & ((1 << s) - 1))
            nacc += s
        run = 0
        for j in range(1, 64):
            v = blk[j]
            if v == 0:
                run += 1
                continue
            while run > 15:
                code, ln = ac[0xF0]
                acc = (acc << ln) | code
                nacc += ln
                run -= 16
            s = abs(v).bit_length()
            code, ln = ac[(run << 4) | s]
            acc = (((acc << ln) | code) << s) | ((v if v >= 0 else v - 1) & ((1 << s) - 1))
            nacc += ln + s
            run = 0
        if run:
            code, ln = ac[0x00]
            acc = (acc << ln) | code
            nacc += ln
        nbytes = nacc >> 3
        if nbytes:
            nacc -= 8 * nbytes
            out += (acc >> nacc).to_bytes(nbytes, "big")
            acc &= (1 << nacc) - 1
    if nacc:
        out.append(((acc << (8 - nacc)) | ((1 << (8 - nacc)) - 1)) & 0xFF)
    return bytes(out).replace(b"\xff", b"\xff\x00")


def encode(frame, quality: int = 95) -> bytes:
    """one complete baseline JFIF file of an HxW (gray) or HxWx3 (BGR) uint8 frame"""
    a = _hwc(frame)
    H, W, C = a.shape
    return headers(H, W, C, quality) + scan_bytes(coefficients(a, quality), C) + b"\xff\xd9"


class RefBackend:
    """the restatement behind jpeg.JpegEncoder's backend seam: encode(frames, on_device, quality) -> list of bytes"""

    def __init__(self):
        self.calls: List[Tuple[int, bool, int]] = []
        self.waits = 0

    def encode(self, frames, on_device: bool, quality: int) -> List[bytes]:
        self.calls.append((len(frames), bool(on_device), int(quality)))
        return [encode(f.cpu().numpy() if on_device else f, quality) for f in frames]

    def wait_stream(self, producer_stream: int) -> None:
        self.waits += 1

    def close(self) -> None:
        pass
