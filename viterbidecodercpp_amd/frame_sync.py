"""Frame synchronisation (BatchDecoder.marker_search / vit_hip_marker_search) and frame extraction (BatchDecoder.frames_extract /
vit_hip_frames_extract): the stock sync markers, the CCSDS randomiser and the rules in numpy.

The device call gives, for every bit phase of the frame period, the Hamming distance of the marker to the decoded bit stream summed
over all frames, and the (phase, polarity) no other beats.  `marker_search_numpy` and `marker_lock_numpy` restate the rule of
include/vit_hip.h on the host, as synth.channel_errors_numpy restates the channel symbol error count.  `frames_extract_numpy` restates
the cut of the stream into byte-aligned frames at that lock, one row at a time, on unpacked bits.
"""
from __future__ import annotations

import numpy as np

CCSDS_ASM = (0x1ACFFC1D, 32)    # the attached sync marker of a CCSDS transfer frame
DVB_SYNC = (0x47, 8)            # the MPEG-2 sync byte of DVB-S, every 204 bytes (every eighth one inverted: search 0x47 at 1632)


def marker_bit_array(marker: int, marker_bits: int) -> np.ndarray:
    """the marker as transmitted: bit j is bit marker_bits-1-j of `marker`"""
    marker, m = int(marker), int(marker_bits)
    if not 1 <= m <= 64 or marker >> m:
        raise ValueError("a marker has 1 to 64 bits and no bit above them")
    return np.array([(marker >> (m - 1 - j)) & 1 for j in range(m)], dtype=np.uint8)


def history_of(bits, marker_bits: int):
    """(history word, history_bits) a search over what FOLLOWS `bits` (0/1, one stream) needs: its last min(m-1, len) bits"""
    bits = np.asarray(bits, dtype=np.uint8).reshape(-1)
    hb = min(int(marker_bits) - 1, bits.size)
    word = 0
    for b in bits[bits.size - hb:]:
        word = (word << 1) | int(b)
    return word, hb


def marker_search_numpy(rows, n_bits: int, marker: int, marker_bits: int, period: int, phase0: int = 0, history=None,
                        history_bits: int = 0):
    """the rule of vit_hip_marker_search: rows [n][>= ceil(n_bits/8)] uint8 (or one row), MSB-first; returns (distance, count), int64
    [n][period]: over the positions -history_bits <= p <= n_bits - marker_bits of phase (phase0 + p) mod period, the number of
    stream bits that differ from the marker and the number of positions.  history [n]: the low history_bits bits are the stream
    bits in front of bit 0, the latest in bit 0."""
    rows = np.asarray(rows, dtype=np.uint8)
    rows = rows[None] if rows.ndim == 1 else rows
    n_bits, m, P, hb = int(n_bits), int(marker_bits), int(period), int(history_bits)
    want = marker_bit_array(marker, m)
    if P < 1 or not 0 <= int(phase0) < P or not 0 <= hb <= 63 or n_bits + hb < m or rows.shape[1] * 8 < n_bits:
        raise ValueError("outside the argument rule of vit_hip_marker_search")
    hist = np.zeros(rows.shape[0], dtype=np.uint64) if history is None else np.asarray(history, dtype=np.uint64).reshape(-1)
    distance = np.zeros((rows.shape[0], P), dtype=np.int64)
    count = np.zeros((rows.shape[0], P), dtype=np.int64)
    phase = (int(phase0) + np.arange(-hb, n_bits - m + 1)) % P
    for r in range(rows.shape[0]):
        before = np.array([(int(hist[r]) >> (hb - 1 - i)) & 1 for i in range(hb)], dtype=np.uint8)
        bits = np.concatenate([before, np.unpackbits(rows[r])[:n_bits]])
        d = (np.lib.stride_tricks.sliding_window_view(bits, m) != want).sum(axis=1)
        distance[r] = np.bincount(phase, weights=d, minlength=P).astype(np.int64)
        count[r] = np.bincount(phase, minlength=P)
    return distance, count


def marker_lock_numpy(distance, count, marker_bits: int) -> np.ndarray:
    """the lock of vit_hip_marker_search from per-phase totals: int64 [n][4] of (phase, inverted, errors, compared).  Candidate
    (phase, upright) has errors = distance, compared = marker_bits * count, (phase, inverted) errors = compared - distance; a beats b
    iff compared_a > 0 and (compared_b == 0 or errors_a * compared_b < errors_b * compared_a); a tie goes to the lower phase, then to
    upright."""
    distance = np.atleast_2d(np.asarray(distance, dtype=np.int64))
    count = np.atleast_2d(np.asarray(count, dtype=np.int64))
    out = np.zeros((distance.shape[0], 4), dtype=np.int64)
    for r in range(distance.shape[0]):
        best = None
        for phase in range(distance.shape[1]):
            compared = int(marker_bits) * int(count[r, phase])
            for inverted, errors in ((0, int(distance[r, phase])), (1, compared - int(distance[r, phase]))):
                if best is None or (compared > 0 and (best[3] == 0 or errors * best[3] < best[2] * compared)):
                    best = (phase, inverted, errors, compared)
        out[r] = best
    return out


def ccsds_randomizer(n_bytes: int) -> np.ndarray:
    """the first n_bytes bytes of the CCSDS pseudo-random sequence (x^8 + x^7 + x^5 + x^3 + 1, the register all ones at the first bit
    behind the sync marker; period 255 bits): FF 48 0E C0 9A 0D 70 BC ...  With drop_bits = 32 it is the `pad` of frames_extract."""
    s = [1] * 8
    bits = np.empty(8 * int(n_bytes), dtype=np.uint8)
    for i in range(bits.size):
        bits[i] = s[0]
        s = s[1:] + [s[0] ^ s[3] ^ s[5] ^ s[7]]
    return np.packbits(bits)


def frames_extract_numpy(row, n_bits: int, period: int, phase0: int, lock, carry=None, carry_bits: int = 0, marker: int = 0,
                         marker_bits: int = 0, drop_bits: int = 0, pad=None):
    """the rule of vit_hip_frames_extract for ONE row: row uint8 [>= ceil(n_bits/8)], lock = (phase, inverted, ...), carry uint8 [>=
    ceil(carry_bits/8)] or None.  returns (frames uint8 [nf][ceil(Q/8)], marker_errors int64 [nf] or None with marker_bits = 0,
    carry_out uint8 [ceil(rem/8)], rem)."""
    n_bits, P, d, m = int(n_bits), int(period), int(drop_bits), int(marker_bits)
    row = np.asarray(row, dtype=np.uint8).reshape(-1)
    if not 8 <= P < 1 << 31 or not 0 <= int(phase0) < P or not 0 <= d < P or n_bits < 1 or row.size * 8 < n_bits or m > min(64, P):
        raise ValueError("outside the argument rule of vit_hip_frames_extract")
    c = int(carry_bits) if carry is not None else 0
    c = 0 if c > P - 1 else c
    before = np.unpackbits(np.asarray(carry, dtype=np.uint8).reshape(-1))[:c] if c else np.zeros(0, dtype=np.uint8)
    S = np.concatenate([before, np.unpackbits(row)[:n_bits]])
    phi, inv = int(lock[0]) % P, np.uint8(int(lock[1]) != 0)
    skip = (phi + c - int(phase0)) % P
    nf, rem = ((S.size - skip) // P, (S.size - skip) % P) if skip < S.size else (0, 0)
    Q = P - d
    F = S[skip:skip + nf * P].reshape(nf, P) ^ inv
    errors = (F[:, :m] != marker_bit_array(marker, m)).sum(axis=1).astype(np.int64) if m else None
    out = F[:, d:]
    if pad is not None:
        out = out ^ np.unpackbits(np.asarray(pad, dtype=np.uint8).reshape(-1))[:Q]
    frames = np.packbits(out, axis=1) if nf else np.zeros((0, (Q + 7) // 8), dtype=np.uint8)
    return frames, errors, np.packbits(S[S.size - rem:] if rem else S[:0]), rem
