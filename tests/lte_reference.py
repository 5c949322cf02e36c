"""An independent restatement of LTE rate matching for the tail-biting code (3GPP TS 36.212 5.1.4.2), its inverse as
vit_hip_lte_rate_dematch_batch defines it (include/vit_hip.h) and the Gold sequence of 36.211 7.2 -- done literally: the interleaver is a
matrix with a NULL sentinel, written by rows, its columns permuted, read by columns, the circular buffer walked entry by entry; the
de-matcher is a scalar loop over k; the Gold sequence runs bit by bit on Python integers.  Nothing here is shared with
viterbidecodercpp_amd/lte.py, and nothing is vectorised."""
import numpy as np

NULL = None
PATTERN = [1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30]
POISON8, POISON16 = 0x5A, 0x5A5A                                   # the fill of an output buffer, as a positive value of its dtype
GUARD = 64                                                         # elements behind an output that must keep the fill


def sub_block(D, i):
    """v(i): the entries (d, i) or NULL of stream i's interleaver, read out column by column"""
    rows = (D + 31) // 32
    y = [NULL] * (32 * rows - D) + [(d, i) for d in range(D)]
    matrix = [[y[32 * r + c] for c in range(32)] for r in range(rows)]             # written row by row
    permuted = [[matrix[r][PATTERN[c]] for c in range(32)] for r in range(rows)]
    return [permuted[r][c] for c in range(32) for r in range(rows)]                # read column by column


def circular_buffer(D):
    return sub_block(D, 0) + sub_block(D, 1) + sub_block(D, 2)


def rate_match_map(D):
    """map[j]: q = 3 d + i of the j-th non-NULL entry of the circular buffer"""
    return [3 * entry[0] + entry[1] for entry in circular_buffer(D) if entry is not NULL]


def rate_match(coded, E):
    """coded: a flat list of 3 D values in decoder order (q = 3 d + i) -> the E transmitted ones, walking the buffer cyclically"""
    D = len(coded) // 3
    w = circular_buffer(D)
    out, at = [], 0
    while len(out) < E:
        entry = w[at % len(w)]
        at += 1
        if entry is not NULL:
            out.append(coded[3 * entry[0] + entry[1]])
    return out


def wrap32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


_MAPS = {}


def dematch(received, frames, D, E_max, stride=0, offsets=None, counts=None, mask_bits=None, period=0, shift=0, lo=-32768, hi=32767):
    """the receive-side rule, one element at a time: received a sequence of ints -> a list of frames x 3 D ints"""
    if D not in _MAPS:
        _MAPS[D] = rate_match_map(D)
    where, n = _MAPS[D], len(received)
    out = []
    for f in range(frames):
        base = int(offsets[f]) if offsets is not None else f * stride
        E = min(int(counts[f]) if counts is not None else E_max, E_max)
        E = 0 if base >= n else min(E, n - base)
        acc = [0] * (3 * D)
        for k in range(E):
            x = int(received[base + k])
            if mask_bits is not None:
                g = (base + k) % period if period else base + k
                if mask_bits[g]:
                    x = -x
            q = where[k % (3 * D)]
            acc[q] = wrap32(acc[q] + x)
        for q in range(3 * D):
            v = wrap32(acc[q] + ((1 << shift) >> 1)) >> shift
            out.append(max(lo, min(hi, v)))
    return out


def gold_bits(c_init, n):
    """c(0 .. n) of 36.211 7.2 on Python integers: bit i of the registers x1, x2 is their element i"""
    x1, x2 = 1, c_init
    bits = []
    for i in range(1600 + n):
        if i >= 1600:
            bits.append((x1 ^ x2) & 1)
        x1 = (x1 >> 1) | ((((x1 >> 3) ^ x1) & 1) << 30)
        x2 = (x2 >> 1) | ((((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1) << 30)
    return bits


def pack_bits(bits):
    """MSB-first bytes of a list of bits"""
    out = bytearray((len(bits) + 7) // 8)
    for t, b in enumerate(bits):
        if b:
            out[t // 8] |= 0x80 >> (t % 8)
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()
