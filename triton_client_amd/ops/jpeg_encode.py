"""JPEG output: the integer definition of the encoder and its GPU op.

The live 2D driver reads ``CompressedImage`` JPEG on the GPU (``ops/jpeg.py``);
this is the other half: annotated frames leave as baseline JFIF files, about a
thirteenth of the raw rgb8 ``Image``.

:func:`encode_numpy` is the specification, in integer arithmetic only, so
``csrc/kernels/jpeg_encode.hip`` reproduces it byte for byte:

* colour: libjpeg ``jccolor`` fixed point (16 fraction bits, its rounding constants);
* chroma: libjpeg's box filters without smoothing (h2v1 ``(a+b+bias)>>1``, bias
  0,1,0,1... along the row; h2v2 ``(a+b+c+d+bias)>>2``, bias 1,2,1,2...);
* edges: pixels outside the image, up to the MCU-padded size, take the nearest edge
  pixel (coordinates are clamped) -- this project's rule; libjpeg fills dummy blocks
  differently, so the two agree on MCU-multiple sizes only;
* DCT: level shift by 128, libjpeg's slow integer FDCT (``jfdctint``, 13-bit constants,
  outputs scaled by 8); quantisation ``q8 = q << 3``, ``(|v| + (q8 >> 1)) / q8``, sign
  restored;
* tables: Annex K base tables under libjpeg's quality rule, clamped to 1..255; the four
  Annex K Huffman tables;
* scan: interleaved MCUs, one restart interval every ``restart`` MCUs (DC prediction
  reset, last byte padded with 1-bits, ``RSTm`` after every interval but the last),
  ``0xFF`` stuffed with ``0x00``;
* file: ``SOI, APP0(JFIF), DQT x2, SOF0, DHT x4, DRI, SOS``, the intervals, ``EOI``.

A restart interval is one independent, byte-aligned unit of work: the device codes
one interval per lane.  The default of 4 MCUs gives a 1280x720 4:2:0 frame 900 of them
(28,800 lanes for the live drivers' batch of 32: about two waves per compute unit; longer
intervals would leave units idle) and costs two marker bytes and up to a byte of padding
per interval: 2.1 % of the stream for the synthetic 1280x720 camera frame at quality 90
(222,989 B against 218,507 B with a single interval).

:class:`JpegBatchEncoder` queues the kernels for a batch of frames on the GPU.
"""
from __future__ import annotations

import io
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from .jpeg import JpegGeometry

SUBSAMPLINGS = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:4": (1, 1)}
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
FORMAT = "rgb8; jpeg compressed bgr8"  # what cli/record.py writes for JPEG topics

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int32)  # natural index of zigzag position k

# Annex K.1 / K.2 base quantisation tables, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int32)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int32)

# Annex K.3 Huffman tables: (codes per length 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
            0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
            0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
            0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
            0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
            0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
            0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
              0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
              0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
              0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
              0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
              0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
              0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFFMAN = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)  # in the file's DHT order: classes/ids 0x00, 0x10, 0x01, 0x11

# offsets of the device table tensor (JpegBatchEncoder.tabs, int32): code << 5 | length per symbol
TAB_DC = (0, 12)
TAB_AC = (24, 280)
TAB_ZIGZAG = 536
TAB_SIZE = 600


@dataclass(frozen=True)
class JpegOptions:
    """What the drivers' ``compressed=`` option carries.  ``cap``: bytes reserved per
    frame on the device path (None: :func:`default_cap`)."""
    quality: int = 90
    subsampling: str = "4:2:0"
    cap: Optional[int] = None
    restart: int = 4


def default_cap(hw: Tuple[int, int]) -> int:
    """H*W*3/4 rounded up to 4 KiB."""
    return -(-(hw[0] * hw[1] * 3 // 4) // 4096) * 4096


def _check(quality: int, subsampling: str, restart: int) -> None:
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"JPEG quality {quality}: 1..100")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"JPEG subsampling {subsampling!r}: one of {sorted(SUBSAMPLINGS)}")
    if not 1 <= int(restart) <= 65535:
        raise ValueError(f"restart interval {restart}: 1..65535 MCUs")


def geometry(hw: Tuple[int, int], subsampling: str = "4:2:0") -> JpegGeometry:
    H, W = int(hw[0]), int(hw[1])
    if not (0 < H <= 65535 and 0 < W <= 65535):
        raise ValueError(f"a JPEG frame is 1..65535 pixels a side, not {W}x{H}")
    hs, vs = SUBSAMPLINGS[subsampling]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    return JpegGeometry(W, H, 3, hs, vs, mcux, mcuy, ((hs, vs), (1, 1), (1, 1)), mcux * mcuy * (hs * vs + 2))


def geometry_record(geo: JpegGeometry) -> np.ndarray:
    """The int32[16] record of csrc/runtime/jpeg_entropy.cpp."""
    return np.array([geo.width, geo.height, geo.nc, geo.hmax, geo.vmax, geo.mcux, geo.mcuy,
                     *[v for hv in geo.sampling for v in hv], geo.nblocks, 0, 0], np.int32)


def quant_tables(quality: int = 90) -> np.ndarray:
    """int32 [2, 64] (luma, chroma), natural order: libjpeg's jpeg_set_quality."""
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)]).astype(np.int32)


def huffman_codes(table) -> dict:
    """symbol -> (code, length), canonical (Annex C)."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


_CODES = [huffman_codes(t) for t in HUFFMAN]  # dc0, ac0, dc1, ac1


def device_tables() -> np.ndarray:
    """int32 [TAB_SIZE]: the four code tables (code << 5 | length, 0: no such symbol) and
    the zigzag order, as ``tca_jpeg_enc_size`` / ``tca_jpeg_enc_write`` read them."""
    t = np.zeros(TAB_SIZE, np.int32)
    for base, codes in ((TAB_DC[0], _CODES[0]), (TAB_AC[0], _CODES[1]), (TAB_DC[1], _CODES[2]), (TAB_AC[1], _CODES[3])):
        for sym, (code, length) in codes.items():
            t[base + sym] = code << 5 | length
    t[TAB_ZIGZAG:] = ZIGZAG
    return t


# ---------------------------------------------------------------------------- pixels -> coefficients
def ycc_planes(rgb: np.ndarray, geo: JpegGeometry) -> List[np.ndarray]:
    """Edge-clamped, colour-converted, downsampled component planes (int32), MCU-padded."""
    H, W = geo.height, geo.width
    PH, PW = geo.mcuy * geo.vmax * 8, geo.mcux * geo.hmax * 8
    yy = np.minimum(np.arange(PH), H - 1)[:, None]
    xx = np.minimum(np.arange(PW), W - 1)[None, :]
    p = rgb[yy, xx].astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    hs, vs = geo.hmax, geo.vmax
    out = [y]
    for c in (cb, cr):
        if hs == 2 and vs == 2:
            bias = 1 + (np.arange(PW // 2) & 1)[None, :]
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        elif hs == 2:
            bias = (np.arange(PW // 2) & 1)[None, :]
            c = (c[:, 0::2] + c[:, 1::2] + bias) >> 1
        out.append(c)
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """One 1-D pass of jfdctint over eight int32 arrays (the samples of a row or column)."""
    t0, t7 = d[0] + d[7], d[0] - d[7]
    t1, t6 = d[1] + d[6], d[1] - d[6]
    t2, t5 = d[2] + d[5], d[2] - d[5]
    t3, t4 = d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15  # CONST_BITS -/+ PASS1_BITS
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o2 = _descale(z1 + t13 * 6270, sh)
    o6 = _descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o7 = _descale(t4 + z1 + z3, sh)
    o5 = _descale(t5 + z2 + z4, sh)
    o3 = _descale(t6 + z2 + z3, sh)
    o1 = _descale(t7 + z1 + z4, sh)
    return [o0, o1, o2, o3, o4, o5, o6, o7]


def fdct_blocks(blocks: np.ndarray) -> np.ndarray:
    """[..., 8, 8] level-shifted int32 samples -> [..., 8, 8] coefficients scaled by 8."""
    rows = np.stack(_fdct_pass([blocks[..., :, k] for k in range(8)], True), -1)
    return np.stack(_fdct_pass([rows[..., k, :] for k in range(8)], False), -2)


def quantize(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    q8 = q.astype(np.int32).reshape(8, 8) << 3
    mag = (np.abs(coef) + (q8 >> 1)) // q8
    return np.where(coef < 0, -mag, mag)


def quantized_coefficients(rgb: np.ndarray, quality: int = 90, subsampling: str = "4:2:0", restart: int = 4):
    """rgb8 [H, W, 3] -> (coef int16 [nblocks, 64] natural order, q int32 [2, 64], geometry);
    block order and geometry are those of ``ops.jpeg.decode_coefficients``."""
    _check(quality, subsampling, restart)
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8:
        raise ValueError(f"rgb8 [H, W, 3] uint8 expected, got {rgb.dtype} {rgb.shape}")
    geo = geometry(rgb.shape[:2], subsampling)
    q = quant_tables(quality)
    parts = []
    for c, plane in enumerate(ycc_planes(rgb, geo)):
        bh, bw = geo.blocks(c)
        blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
        parts.append(quantize(fdct_blocks(blocks), q[min(c, 1)]).reshape(bh * bw, 64))
    return np.concatenate(parts).astype(np.int16), q, geo


# ---------------------------------------------------------------------------- coefficients -> bytes
def mcu_blocks(geo: JpegGeometry, mcu: int) -> List[Tuple[int, int]]:
    """(component, block index in the planar order) of one MCU's blocks, in scan order."""
    my, mx = divmod(mcu, geo.mcux)
    out, off = [], 0
    for c in range(geo.nc):
        h, v = geo.sampling[c]
        bh, bw = geo.blocks(c)
        out += [(c, off + (my * v + dy) * bw + mx * h + dx) for dy in range(v) for dx in range(h)]
        off += bh * bw
    return out


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


def scan_tokens(coef: np.ndarray, geo: JpegGeometry, restart: int = 4) -> List[List[tuple]]:
    """The entropy-coded symbols per restart interval: (table, symbol, bits, nbits) with
    table 0..3 = DC luma, AC luma, DC chroma, AC chroma and ``bits`` the ``nbits`` extra
    bits that follow the symbol's code."""
    nm = geo.mcux * geo.mcuy
    zz = coef[:, ZIGZAG].astype(np.int64)
    segs = []
    for s in range(0, nm, restart):
        toks, pred = [], [0] * geo.nc
        for mcu in range(s, min(s + restart, nm)):
            for c, bi in mcu_blocks(geo, mcu):
                tb = 0 if c == 0 else 2
                blk = [int(v) for v in zz[bi]]
                d = blk[0] - pred[c]
                pred[c] = blk[0]
                n = _category(d)
                toks.append((tb, n, (d if d >= 0 else d - 1) & ((1 << n) - 1), n))
                run = 0
                for v in blk[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        toks.append((tb + 1, 0xF0, 0, 0))
                        run -= 16
                    n = _category(v)
                    if n > 10:
                        raise ValueError(f"AC coefficient {v} does not fit a baseline JPEG")
                    toks.append((tb + 1, run << 4 | n, (v if v >= 0 else v - 1) & ((1 << n) - 1), n))
                    run = 0
                if run:
                    toks.append((tb + 1, 0x00, 0, 0))
        segs.append(toks)
    return segs


def segment_bytes(tokens: Sequence[tuple]) -> bytes:
    """One restart interval's bytes: codes, 1-bit padding, 0xFF stuffing (no marker)."""
    acc, nb = 0, 0
    for tb, sym, bits, n in tokens:
        code, length = _CODES[tb][sym]
        acc = (acc << (length + n)) | (code << n) | bits
        nb += length + n
    pad = -nb % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    raw = acc.to_bytes((nb + pad) // 8, "big")
    return raw.replace(b"\xff", b"\xff\x00")


def _seg(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header_bytes(width: int, height: int, quality: int = 90, subsampling: str = "4:2:0", restart: int = 4) -> bytes:
    """Everything before the entropy-coded data; depends on these five values only."""
    _check(quality, subsampling, restart)
    geo = geometry((height, width), subsampling)
    q = quant_tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += _seg(0xDB, bytes([i]) + bytes(int(v) for v in q[i][ZIGZAG]))
    comps = b"".join(bytes([c + 1, geo.sampling[c][0] << 4 | geo.sampling[c][1], min(c, 1)]) for c in range(3))
    out += _seg(0xC0, b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03" + comps)
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), HUFFMAN):
        out += _seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _seg(0xDD, int(restart).to_bytes(2, "big"))
    return out + _seg(0xDA, b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")


def encode_coefficients(coef: np.ndarray, geo: JpegGeometry, quality: int, subsampling: str, restart: int) -> bytes:
    segs = [segment_bytes(t) for t in scan_tokens(coef, geo, restart)]
    body = b"".join(s + bytes([0xFF, 0xD0 + (i & 7)]) for i, s in enumerate(segs[:-1])) + segs[-1]
    return header_bytes(geo.width, geo.height, quality, subsampling, restart) + body + b"\xff\xd9"


def encode_numpy(rgb: np.ndarray, quality: int = 90, subsampling: str = "4:2:0", restart: int = 4) -> bytes:
    """rgb8 [H, W, 3] -> a baseline JFIF file (the definition of the device encoder)."""
    coef, _, geo = quantized_coefficients(rgb, quality, subsampling, restart)
    return encode_coefficients(coef, geo, quality, subsampling, restart)


def encode_pil(rgb: np.ndarray, quality: int = 90, subsampling: str = "4:2:0") -> bytes:
    """The drivers' host path (engines without a device live path, and frames that
    overflow the device path's ``cap``): libjpeg through PIL."""
    from PIL import Image

    _check(quality, subsampling, 1)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, format="JPEG", quality=int(quality),
                                                   subsampling=PIL_SUBSAMPLING[subsampling])
    return buf.getvalue()


# ---------------------------------------------------------------------------- the GPU op
class JpegBatchEncoder:
    """uint8 RGB NHWC frames on the GPU -> one JFIF file per frame, on the GPU.

    Owns the coefficient, interval-size, interval-offset, table and header tensors;
    :meth:`encode_` queues ``tca_jpeg_fdct``, ``tca_jpeg_enc_size``, ``tca_jpeg_enc_scan``
    and ``tca_jpeg_enc_write`` (``csrc/kernels/jpeg_encode.hip``) on one stream: fixed
    grids, no host reads, so the call can be captured in a graph."""

    def __init__(self, batch: int, hw: Tuple[int, int], device, quality: int = 90, subsampling: str = "4:2:0",
                 restart: int = 4, cap: Optional[int] = None):
        _check(quality, subsampling, restart)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("JpegBatchEncoder runs on the GPU; on the host use encode_pil / encode_numpy")
        self.B, self.hw = int(batch), (int(hw[0]), int(hw[1]))
        self.quality, self.subsampling, self.restart = int(quality), subsampling, int(restart)
        self.geo = geo = geometry(self.hw, subsampling)
        self.cap = int(cap) if cap else default_cap(self.hw)
        self.header = header_bytes(geo.width, geo.height, quality, subsampling, restart)
        self.nseg = -(-geo.mcux * geo.mcuy // self.restart)
        self.geom_rec = geometry_record(geo)
        dev = self.device
        self.hdr = torch.frombuffer(bytearray(self.header), dtype=torch.uint8).to(dev)
        self.qt = torch.from_numpy(quant_tables(quality)).to(dev)
        self.tabs = torch.from_numpy(device_tables()).to(dev)
        self.coef = torch.empty((self.B, geo.nblocks, 64), dtype=torch.int16, device=dev)
        self.seg_size = torch.empty((self.B, self.nseg), dtype=torch.int32, device=dev)
        self.seg_off = torch.empty((self.B, self.nseg), dtype=torch.int32, device=dev)

    def buffers(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """A fresh (out uint8 [B, cap], lens int32 [B]) pair on the device."""
        return (torch.zeros((self.B, self.cap), dtype=torch.uint8, device=self.device),
                torch.zeros((self.B,), dtype=torch.int32, device=self.device))

    def fdct_(self, frames: torch.Tensor, n: Optional[int] = None, stream=None) -> torch.Tensor:
        """Quantised coefficients of ``frames[:n]`` into ``self.coef`` (returned)."""
        self._fdct(frames, self._check_frames(frames, n), stream)
        return self.coef

    def _fdct(self, frames: torch.Tensor, n: int, stream) -> None:
        H, W = self.hw
        _native.call("tca_jpeg_fdct", frames.data_ptr(), self.qt.data_ptr(), self.coef.data_ptr(),
                     self.geom_rec.ctypes.data, H * W * 3, self.geo.nblocks, n, _native.stream_ptr(stream))

    def _check_frames(self, frames: torch.Tensor, n: Optional[int]) -> int:
        H, W = self.hw
        if not frames.is_cuda:
            raise ValueError("JpegBatchEncoder takes GPU frames; on the host use encode_pil / encode_numpy")
        if (frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (H, W, 3)
                or not frames.is_contiguous() or frames.device != self.coef.device):
            raise ValueError(f"frames must be contiguous uint8 [n, {H}, {W}, 3] on {self.coef.device}, got "
                             f"{frames.dtype} {tuple(frames.shape)} on {frames.device}")
        n = frames.shape[0] if n is None else int(n)
        if not 0 < n <= min(self.B, frames.shape[0]):
            raise ValueError(f"{n} frames for an encoder of {self.B} and {frames.shape[0]} frames given")
        return n

    def encode_(self, frames: torch.Tensor, out: torch.Tensor, lens: torch.Tensor, n: Optional[int] = None,
                stream=None) -> None:
        """frames[:n] -> out[b, :lens[b]] = frame b's file; a frame that needs more than
        ``out``'s row reports ``lens[b] = -needed`` and its row is left untouched."""
        n = self._check_frames(frames, n)
        for t, dt in ((out, torch.uint8), (lens, torch.int32)):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.device != self.coef.device:
                raise ValueError("out / lens must be contiguous uint8 [n, cap] / int32 [n] tensors on the encoder's GPU")
        if out.dim() != 2 or out.shape[0] < n or lens.numel() < n:
            raise ValueError(f"out {tuple(out.shape)} / lens {tuple(lens.shape)} hold fewer than {n} frames")
        cap, st = int(out.shape[1]), _native.stream_ptr(stream)
        self._fdct(frames, n, stream)
        rec, nb, ns = self.geom_rec.ctypes.data, self.geo.nblocks, self.nseg
        _native.call("tca_jpeg_enc_size", self.coef.data_ptr(), self.tabs.data_ptr(), rec, nb, self.restart,
                     self.seg_size.data_ptr(), ns, n, st)
        _native.call("tca_jpeg_enc_scan", self.seg_size.data_ptr(), self.seg_off.data_ptr(), ns, self.hdr.data_ptr(),
                     self.hdr.numel(), out.data_ptr(), cap, lens.data_ptr(), n, st)
        _native.call("tca_jpeg_enc_write", self.coef.data_ptr(), self.tabs.data_ptr(), rec, nb, self.restart,
                     self.seg_off.data_ptr(), ns, self.hdr.numel(), out.data_ptr(), cap, lens.data_ptr(), n, st)
