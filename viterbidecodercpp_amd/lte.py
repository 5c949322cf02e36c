"""The front of the LTE control-channel route: the rate matching of the tail-biting code (3GPP TS 36.212 5.1.4.2) as
vit_hip_lte_rate_dematch_batch undoes it (include/vit_hip.h) -- the map, the transmit side (lte_rate_match_numpy), the rule of the
receive side on the host (lte_rate_dematch_numpy) --, the Gold sequence of the scrambler (36.211 7.2) and the aligned PDCCH candidates of
a control region.  The GPU side is BatchDecoder.lte_rate_dematch (decoder.py)."""
from __future__ import annotations

import numpy as np

# table 5.1.4-2: the inter-column permutation of the sub-block interleaver for convolutionally coded channels (not the turbo one)
LTE_CC_COLUMN_PERMUTATION = (1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30)
LTE_MAX_D = 8192


def lte_rate_match_map(D: int):
    """map[j], j in [0, 3D): the decoder-order index q = 3 d + i (i the polynomial index, the last axis of [D][3]) of the j-th non-NULL
    entry of the circular buffer w = v(0) | v(1) | v(2); transmitted bit k is coded bit map[k mod 3D].  int32 [3D]"""
    D = int(D)
    if D < 1:
        raise ValueError("D must be at least 1")
    rows = -(-D // 32)
    y = np.concatenate([np.full(32 * rows - D, -1, dtype=np.int64), np.arange(D, dtype=np.int64)])
    v = y.reshape(rows, 32)[:, list(LTE_CC_COLUMN_PERMUTATION)].T.reshape(-1)          # columns permuted, read column by column
    v = v[v >= 0]
    return np.concatenate([3 * v + i for i in range(3)]).astype(np.int32)


def lte_rate_match_numpy(coded, E: int):
    """the transmit side: coded [..., D, 3] -> the E transmitted elements [..., E], e[k] = coded[map[k mod 3D]] (repeated where E > 3D,
    punctured where E < 3D)"""
    coded = np.asarray(coded)
    if coded.ndim < 2 or coded.shape[-1] != 3:
        raise ValueError("coded must be [..., D, 3]")
    n3 = 3 * coded.shape[-2]
    idx = lte_rate_match_map(coded.shape[-2])[np.arange(int(E)) % n3]
    return np.ascontiguousarray(coded.reshape(coded.shape[:-2] + (n3,))[..., idx])     # the index leaves the last axis strided


def lte_rate_dematch_numpy(received, frames: int, D: int, E_max: int, received_frame_stride: int = 0, offsets=None, counts=None,
                           scramble=None, scramble_period: int = 0, shift: int = 0, clamp_lo: int = -32768, clamp_hi: int = 32767):
    """the rule of vit_hip_lte_rate_dematch_batch on the host: received, a 1-D int8 / int16 array of n_received elements, -> [frames][D][3]
    of its dtype.  Frame f starts at offsets[f] (None: f * received_frame_stride) and holds min(counts[f], E_max) elements (None:
    E_max), cut at the end of `received`; scramble: the mask as packed bytes, MSB-first (None: off), its bit for element g being g mod
    scramble_period (0: g).  Sums, the negation and the rounding add are int32 (modulo 2^32)."""
    received = np.asarray(received)
    if received.ndim != 1 or received.dtype not in (np.int8, np.int16):
        raise ValueError("received must be a 1-D int8 or int16 array")
    frames, D, E_max, shift, period = int(frames), int(D), int(E_max), int(shift), int(scramble_period)
    info = np.iinfo(received.dtype)
    if not 1 <= D <= LTE_MAX_D or not 1 <= E_max < 1 << 24 or not 0 <= shift <= 15 or not info.min <= clamp_lo <= clamp_hi <= info.max:
        raise ValueError("D must be 1 .. 8192, E_max 1 .. 2^24 - 1, shift 0 .. 15, the clamp a range of the dtype")
    n, n3 = received.size, 3 * D
    if offsets is None and frames and (received_frame_stride < E_max or (frames - 1) * received_frame_stride + E_max > n):
        raise ValueError("the frames do not lie inside received")
    where = lte_rate_match_map(D)
    bits = None if scramble is None else np.unpackbits(np.asarray(scramble, dtype=np.uint8))
    out = np.empty((frames, n3), dtype=received.dtype)
    for f in range(frames):
        base = int(offsets[f]) if offsets is not None else f * int(received_frame_stride)
        E = min(E_max if counts is None else int(counts[f]), E_max, max(n - base, 0))
        x = received[base:base + E].astype(np.int64)
        if bits is not None and E:
            g = base + np.arange(E)
            x = np.where(bits[g % period if period else g] != 0, -x, x)
        wraps = -(-E // n3)
        sums = np.concatenate([x, np.zeros(wraps * n3 - E, dtype=np.int64)]).reshape(wraps, n3).sum(axis=0) if wraps else np.zeros(n3, dtype=np.int64)
        acc = np.zeros(n3, dtype=np.int64)
        acc[where] = sums
        acc = (acc + ((1 << shift) >> 1)).astype(np.int32) >> shift                    # int32, modulo 2^32; the shift is arithmetic
        out[f] = np.clip(acc, clamp_lo, clamp_hi)
    return out.reshape(frames, D, 3)


def lte_gold_sequence(c_init: int, n: int):
    """the length-31 Gold sequence of 36.211 7.2, c(0 .. n): c(i) = x1(i + 1600) ^ x2(i + 1600), x1(i+31) = x1(i+3) ^ x1(i) from x1(0) = 1,
    x2(i+31) = x2(i+3) ^ x2(i+2) ^ x2(i+1) ^ x2(i) from the bits of c_init (bit i of c_init is x2(i)).  returns (bytes, bits): the mask
    packed MSB-first as vit_hip_lte_rate_dematch_batch takes it, uint8 [ceil(n/8)], and the bits, uint8 [n]"""
    c_init, n = int(c_init), int(n)
    if not 0 <= c_init < 1 << 31 or n < 0:
        raise ValueError("c_init must lie in 0 .. 2^31 - 1, n must not be negative")
    total = 1600 + n
    x1, x2 = np.zeros(total + 31, dtype=np.uint8), np.zeros(total + 31, dtype=np.uint8)
    x1[0] = 1
    x2[:31] = (c_init >> np.arange(31)) & 1
    for i in range(total):
        x1[i + 31] = x1[i + 3] ^ x1[i]
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    bits = x1[1600:total] ^ x2[1600:total]
    return np.packbits(bits), bits


def pdcch_candidates(n_cce: int, levels=(1, 2, 4, 8)):
    """every aligned PDCCH candidate of a control region of n_cce control channel elements (72 soft bits each): for every aggregation
    level L of `levels` and every m < n_cce // L, 72 L soft bits at offset 72 L m.  returns (offsets, counts), uint32 arrays, level by
    level -- d_offset and d_count of vit_hip_lte_rate_dematch_batch with E_max = 72 max(levels)"""
    n_cce = int(n_cce)
    if n_cce < 0 or any(int(L) < 1 for L in levels):
        raise ValueError("n_cce must not be negative, levels at least 1")
    offsets = [72 * int(L) * m for L in levels for m in range(n_cce // int(L))]
    counts = [72 * int(L) for L in levels for m in range(n_cce // int(L))]
    return np.asarray(offsets, dtype=np.uint32), np.asarray(counts, dtype=np.uint32)
