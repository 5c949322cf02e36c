"""An independent restatement of the CRC rule of vit_hip_crc_batch (include/vit_hip.h), for the tests of both tiers: the data bits as ONE
Python integer, divided by the generator as polynomials over GF(2) -- crc = (m(x) x^width + init x^n) mod P(x) ^ xorout --, a different
arithmetic from the bit-serial register of viterbidecodercpp_amd.crc.crc_numpy and from the tables of the kernel.  And the case maker
both tiers share: frames in a buffer with an odd base address and stride, a guard value around them, and the images of both outputs."""
import functools

import numpy as np

from viterbidecodercpp_amd import CRCCode

POISON, POISON32, GUARD = 0xA5, 0xA5A5A5A5, 0x5A
WIDTHS_CPU = (1, 3, 5, 8, 12, 16, 24, 31, 32)
WIDTHS_GPU = (1, 5, 8, 16, 24, 31, 32)
FIRST_BITS = (0, 1, 7, 8, 13)
# the lengths the issue names, and one on either side of every length at which the host rule doubles the lanes of a frame (16 bytes a
# lane: 128 | 129 bits, 256 | 257, ... 4096 | 4097), and the first whole byte past each
N_BITS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 240, 8904, 32771)
N_BITS_G = (128, 129, 136, 256, 257, 264, 512, 513, 520, 1024, 1025, 1032, 2048, 2049, 2056, 4096, 4097, 4104)


def polymod(value: int, nbits: int, generator: int, width: int) -> int:
    """value(x) mod generator(x) over GF(2): `value` has nbits bits, `generator` carries its x^width term.  Long division, 64 quotient
    bits at a time from the top so that the running remainder stays small"""
    rem = 0
    for lo in range((nbits - 1) // 64 * 64 if nbits else 0, -1, -64):
        take = min(64, nbits - lo)
        rem = (rem << take) | ((value >> lo) & ((1 << take) - 1))
        for k in range(rem.bit_length() - 1, width - 1, -1):
            if (rem >> k) & 1:
                rem ^= generator << (k - width)
    return rem


def bits_int(frame, first: int, n: int) -> int:
    """bits [first, first + n) of the uint8 array `frame` as an integer, bit `first` the highest"""
    whole = int.from_bytes(bytes(bytearray(frame)), "big")
    return (whole >> (8 * len(frame) - first - n)) & ((1 << n) - 1)


def crc_reference(code: CRCCode, frame, n_bits: int, first_bit: int = 0) -> int:
    m = bits_int(frame, first_bit, n_bits)
    generator = (1 << code.width) | code.poly
    return polymod((m << code.width) ^ (code.init << n_bits), n_bits + code.width, generator, code.width) ^ code.xorout


def field_reference(code: CRCCode, frame, n_bits: int, first_bit: int = 0) -> int:
    return bits_int(frame, first_bit + n_bits, code.width)


def random_code(width: int, rng) -> CRCCode:
    top = 1 << width
    return CRCCode(width, int(rng.integers(0, top)), int(rng.integers(0, top)), int(rng.integers(0, top)))


@functools.lru_cache(maxsize=None)
def make_case(width: int, n_bits: int, first_bit: int, rows: int, max_frames: int, field: bool = True, lead: int = 1, slack: int = 3,
              counts=None, seed: int = 0):
    """a case of vit_hip_crc_batch for a random code of `width`: a dict with
      code, rows, max_frames, n_bits, first_bit, field, lead, counts (a tuple per row, or None: all frames)
      stride    need + slack bytes, need = ceil((first_bit + n_bits (+ width)) / 8)
      buffer    uint8 [lead + (rows * max_frames - 1) * stride + need]: frame (r, f) at lead + (r * max_frames + f) * stride; the bytes
                in front and the slack between frames hold GUARD, the last frame ends the buffer
      crc, syndrome   int64 [rows][max_frames]: the images of the outputs over a POISON32 fill (syndrome: all POISON32 without field)
    Cached: the tests share a case and must not change it."""
    rng = np.random.default_rng([width, n_bits, first_bit, rows, max_frames, int(field), seed])
    code = random_code(width, rng)
    need = (first_bit + n_bits + (width if field else 0) + 7) // 8
    stride = need + slack
    N = rows * max_frames
    buffer = np.full(lead + (N - 1) * stride + need, GUARD, dtype=np.uint8)
    crc = np.full((rows, max_frames), POISON32, dtype=np.int64)
    syndrome = np.full((rows, max_frames), POISON32, dtype=np.int64)
    for r in range(rows):
        nf = max_frames if counts is None else min(counts[r], max_frames)
        for f in range(max_frames):
            at = lead + (r * max_frames + f) * stride
            buffer[at:at + need] = rng.integers(0, 256, size=need, dtype=np.uint8)
            if f < nf:
                frame = buffer[at:at + need]
                crc[r, f] = crc_reference(code, frame, n_bits, first_bit)
                if field:
                    syndrome[r, f] = crc[r, f] ^ field_reference(code, frame, n_bits, first_bit)
    buffer.setflags(write=False), crc.setflags(write=False), syndrome.setflags(write=False)
    return dict(code=code, rows=rows, max_frames=max_frames, n_bits=n_bits, first_bit=first_bit, field=field, lead=lead, counts=counts,
                stride=stride, need=need, buffer=buffer, crc=crc, syndrome=syndrome)


def frames_of(case):
    """the frames of a case as a uint8 array [rows][max_frames][need] (a copy)"""
    N, s, need = case["rows"] * case["max_frames"], case["stride"], case["need"]
    idx = case["lead"] + np.arange(N)[:, None] * s + np.arange(need)[None, :]
    return case["buffer"][idx].reshape(case["rows"], case["max_frames"], need)
