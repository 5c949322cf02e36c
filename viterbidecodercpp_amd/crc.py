"""The frame check: CRC codes as vit_hip_crc_batch takes them (include/vit_hip.h) -- not reflected, bits MSB-first -- with the rule on
the host (crc_numpy) and the transmit side (crc_append_numpy).  The GPU side is BatchDecoder.crc_check (outer.py)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class CRCCode:
    """(width, poly, init, xorout): 1 <= width <= 32, poly without its x^width term, all three below 2^width"""
    width: int
    poly: int
    init: int = 0
    xorout: int = 0

    def __post_init__(self):
        for name in ("width", "poly", "init", "xorout"):
            value = getattr(self, name)
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                raise ValueError(f"{name} must be an integer")
            object.__setattr__(self, name, int(value))
        if not 1 <= self.width <= 32:
            raise ValueError("width must be 1 .. 32")
        for name in ("poly", "init", "xorout"):
            if not 0 <= getattr(self, name) < 1 << self.width:
                raise ValueError(f"{name} must lie in 0 .. 2^width - 1")


CCSDS_CRC16 = CRCCode(16, 0x1021, 0xFFFF, 0)          # the frame error control field of a transfer frame (CCSDS 132.0-B)
LTE_CRC16 = CRCCode(16, 0x1021, 0, 0)                 # gCRC16 (3GPP TS 36.212): PBCH, PDCCH
DAB_CRC16 = CRCCode(16, 0x1021, 0xFFFF, 0xFFFF)       # behind the 30 data bytes of a FIB (EN 300 401)
LTE_CRC24A = CRCCode(24, 0x864CFB, 0, 0)
LTE_CRC24B = CRCCode(24, 0x800063, 0, 0)
LTE_CRC8 = CRCCode(8, 0x9B, 0, 0)
MPEG2_CRC32 = CRCCode(32, 0x04C11DB7, 0xFFFFFFFF, 0)  # PSI sections (ISO/IEC 13818-1)
# the 802.11 FCS over bits in transmit order (octets LSB first): zlib.crc32 of the octets is the 32-bit reversal of this code's value
WIFI_FCS = CRCCode(32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF)
STOCK_CRC_CODES = {"CCSDS_CRC16": CCSDS_CRC16, "LTE_CRC16": LTE_CRC16, "DAB_CRC16": DAB_CRC16, "LTE_CRC24A": LTE_CRC24A,
                   "LTE_CRC24B": LTE_CRC24B, "LTE_CRC8": LTE_CRC8, "MPEG2_CRC32": MPEG2_CRC32}


def _bits(frames, first, n, what):
    """bits [first, first + n) of every frame of a uint8 array [...][bytes], as uint8 0/1 [...][n]"""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim < 1:
        raise ValueError("frames must be a uint8 array [...][bytes]")
    first, n = int(first), int(n)
    if first < 0 or n < 0 or first + n > 8 * frames.shape[-1]:
        raise ValueError(f"{what} lie outside the {frames.shape[-1]} bytes of a frame")
    lo, hi = first // 8, (first + n + 7) // 8
    return np.unpackbits(frames[..., lo:hi], axis=-1)[..., first - 8 * lo:first - 8 * lo + n]


def crc_numpy(code: CRCCode, frames, n_bits: int, first_bit: int = 0):
    """the rule of vit_hip_crc_batch, vectorised over frames: the CRC of bits [first_bit, first_bit + n_bits) of every frame of the uint8
    array [...][bytes] (bit t of a frame is bit 7 - t%8 of byte t/8), as int64 [...]"""
    bits = _bits(frames, first_bit, n_bits, "the data bits")
    mask, top = (1 << code.width) - 1, code.width - 1
    reg = np.full(bits.shape[:-1], code.init, dtype=np.int64)
    for k in range(bits.shape[-1]):
        fb = ((reg >> top) & 1) ^ bits[..., k]
        reg = ((reg << 1) & mask) ^ (fb * code.poly)
    return reg ^ code.xorout


def crc_field_numpy(code: CRCCode, frames, n_bits: int, first_bit: int = 0):
    """the transmitted field: the code.width bits behind the data of every frame, MSB-first, as int64 [...]"""
    bits = _bits(frames, int(first_bit) + int(n_bits), code.width, "the field bits").astype(np.int64)
    return (bits << np.arange(code.width - 1, -1, -1)).sum(axis=-1)


def crc_append_numpy(code: CRCCode, frames, n_bits: int, first_bit: int = 0, mask=0):
    """the transmit side: a copy of `frames` (uint8 [...][bytes], lengthened with zero bytes where the field needs them) with the CRC of
    bits [first_bit, first_bit + n_bits), XORed with `mask` (an int or an array [...]: the RNTI, say), written into the code.width bits
    behind them.  crc_numpy ^ crc_field_numpy of the result -- the syndrome of vit_hip_crc_batch -- is `mask`"""
    frames = np.asarray(frames)
    first_bit, n_bits = int(first_bit), int(n_bits)
    value = crc_numpy(code, frames, n_bits, first_bit) ^ np.asarray(mask, dtype=np.int64)
    if ((value >> code.width) != 0).any():
        raise ValueError("mask must lie below 2^width")
    end = first_bit + n_bits
    need = (end + code.width + 7) // 8
    out = np.zeros(frames.shape[:-1] + (max(need, frames.shape[-1]),), dtype=np.uint8)
    out[..., :frames.shape[-1]] = frames
    lo = end // 8
    bits = np.unpackbits(out[..., lo:need], axis=-1)
    bits[..., end - 8 * lo:end - 8 * lo + code.width] = (value[..., None] >> np.arange(code.width - 1, -1, -1)) & 1
    out[..., lo:need] = np.packbits(bits, axis=-1)
    return out
