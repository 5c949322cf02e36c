"""The DVB-S outer chain around Reed-Solomon (BatchDecoder.deinterleave / vit_hip_deinterleave_batch and BatchDecoder.dvb_derandomize /
vit_hip_dvb_derandomize_batch): the interleaver's parameters, the energy-dispersal sequence and both rules in numpy, with the
transmit side of either for tests and users.

A DVB-S transmitter scrambles every 188-byte transport packet with a sequence that restarts every eighth packet, where it inverts the
sync byte (0x47 -> 0xB8); appends 16 Reed-Solomon bytes (reed_solomon.DVB_RS_204_188); and sends the 204 bytes through a convolutional
(Forney) interleaver of 12 branches whose delays grow by 17 bytes, the sync byte on the branch without delay.  The receiver undoes the
three in the reverse order.
"""
from __future__ import annotations

import functools

import numpy as np

DVB_INTERLEAVER = (12, 17)      # (branches, cell): branch j delays by 17 j bytes of its own, 12 * 17 j bytes of the stream
DVB_PACKET = 188                # an MPEG-2 transport packet
_ALL_ONES = 0xFFFFFFFF          # d_phase_out of a row whose group phase is still unknown


@functools.lru_cache(maxsize=None)
def _prbs() -> np.ndarray:
    reg = [int(c) for c in "100101010000000"]                     # registers 1 .. 15
    bits = np.empty(8 * 1503, dtype=np.uint8)
    for i in range(bits.size):
        out = reg[13] ^ reg[14]
        bits[i] = out
        reg = [out] + reg[:-1]
    seq = np.packbits(bits)
    seq.setflags(write=False)
    return seq


def dvb_prbs() -> np.ndarray:
    """the 1503 bytes of the energy-dispersal sequence (EN 300 421: 1 + x^14 + x^15, registers loaded with 100101010000000, MSB-first):
    03 F6 08 34 30 B8 A3 93 ...  Byte 188 q + i - 1 belongs to byte i >= 1 of packet q of a group of eight."""
    return _prbs().copy()


def history_packets(branches: int, cell: int, packet_bytes: int) -> int:
    """H = ceil((B-1) M B / n): the packets the de-interleaver's output lags its input by"""
    B, M, n = int(branches), int(cell), int(packet_bytes)
    if B < 2 or M < 1 or n < 1 or n % B:
        raise ValueError("branches must be at least 2, cell at least 1, packet_bytes a multiple of branches")
    return -(-(B - 1) * M * B // n)


def conv_interleave_numpy(packets, branches: int, cell: int) -> np.ndarray:
    """the transmit side: packets uint8 [N][n] -> [N][n], byte i of the stream delayed by (i mod B) M B bytes; what the delay lines
    hold at the start (zeros) fills the places in front.  conv_deinterleave_numpy of the result is the byte stream of `packets` delayed
    by D = (B-1) M B bytes: by H whole packets where n divides D, as in DVB-S."""
    x = np.asarray(packets, dtype=np.uint8)
    history_packets(branches, cell, x.shape[1])                   # the argument rule
    flat = x.reshape(-1)
    at = np.arange(flat.size)
    src = at - (at % int(branches)) * int(cell) * int(branches)
    return np.where(src >= 0, flat[np.maximum(src, 0)], 0).astype(np.uint8).reshape(x.shape)


def conv_deinterleave_numpy(packets, branches: int, cell: int, hist=None, fill: int = 0, n_frames: int = None):
    """the rule of vit_hip_deinterleave_batch for ONE row: packets uint8 [>= nf][n], hist uint8 [H][n] or None, of which the last
    min(fill, H) packets are real.  returns (out uint8 [nout][n], nout, hist uint8 [H][n] -- the packets in front of the real ones zero
    --, fill)."""
    x = np.asarray(packets, dtype=np.uint8)
    B, M, n = int(branches), int(cell), int(x.shape[1])
    H = history_packets(B, M, n)
    nf = x.shape[0] if n_frames is None else min(int(n_frames), x.shape[0])
    fill = min(int(fill), H) if hist is not None else 0
    old = np.asarray(hist, dtype=np.uint8).reshape(H, n)[H - fill:] if fill else np.zeros((0, n), dtype=np.uint8)
    S = np.concatenate([old, x[:nf]])
    T = S.shape[0]
    nout = max(0, T - H)
    Sb = S.reshape(-1)
    i = np.arange(n)
    back = (B - 1 - i % B) * M * B
    out = np.zeros((nout, n), dtype=np.uint8)
    for k in range(nout):
        out[k] = Sb[(H + k) * n + i - back]
    keep = min(H, T)
    new = np.zeros((H, n), dtype=np.uint8)
    if keep:
        new[H - keep:] = S[T - keep:]
    return out, nout, new, keep


def dvb_randomize_numpy(packets, phase: int = 0) -> np.ndarray:
    """the transmit side: transport packets uint8 [N][188] -> [N][188], packet f at place q = (phase + f) mod 8 of its group: byte 0
    inverted where q = 0, bytes 1 .. 187 XORed with the sequence"""
    x = np.asarray(packets, dtype=np.uint8)
    if x.ndim != 2 or x.shape[1] != DVB_PACKET:
        raise ValueError("packets must be [N][188]")
    prbs = _prbs()
    out = x.copy()
    for f in range(x.shape[0]):
        q = (int(phase) + f) % 8
        if q == 0:
            out[f, 0] ^= 0xFF
        out[f, 1:] ^= prbs[DVB_PACKET * q:DVB_PACKET * q + DVB_PACKET - 1]
    return out


def dvb_phase_vote_numpy(sync_bytes) -> int:
    """the group phase the sync bytes of a call name: the g with the fewest bits of in[f][0] ^ (0xB8 if (g + f) mod 8 = 0 else 0x47), the
    lower g on a tie; 8 (unknown) without a packet"""
    s = np.asarray(sync_bytes, dtype=np.uint8).reshape(-1)
    if s.size == 0:
        return 8
    f = np.arange(s.size)
    costs = []
    for g in range(8):
        want = np.where((g + f) % 8 == 0, 0xB8, 0x47).astype(np.uint8)
        costs.append(int(np.unpackbits(s ^ want).sum()))
    return int(np.argmin(costs))


def dvb_derandomize_numpy(packets, phase=None, rs_status=None, n_frames: int = None):
    """the rule of vit_hip_dvb_derandomize_batch for ONE row: packets uint8 [>= nf][>= 188], phase 0 .. 7 or None / >= 8: unknown (voted
    from the sync bytes), rs_status int [>= nf] or None.  returns (out uint8 [nf][188], sync_errors int64 [nf], phase_out: (g + nf) mod
    8, or 0xFFFFFFFF while unknown)."""
    x = np.asarray(packets, dtype=np.uint8)
    if x.ndim != 2 or x.shape[1] < DVB_PACKET:
        raise ValueError("packets must be [N][>= 188]")
    nf = x.shape[0] if n_frames is None else min(int(n_frames), x.shape[0])
    x = x[:nf, :DVB_PACKET]
    g = 8 if phase is None or not 0 <= int(phase) < 8 else int(phase)
    if g >= 8:
        g = dvb_phase_vote_numpy(x[:, 0])
    if g >= 8:
        return np.zeros((0, DVB_PACKET), dtype=np.uint8), np.zeros(0, dtype=np.int64), _ALL_ONES
    q = (g + np.arange(nf)) % 8
    want = np.where(q == 0, 0xB8, 0x47).astype(np.uint8)
    errors = np.unpackbits((x[:, 0] ^ want)[:, None], axis=1).sum(axis=1).astype(np.int64)
    out = dvb_randomize_numpy(x, g)                               # the sequence is its own inverse
    if rs_status is not None:
        out[np.asarray(rs_status).reshape(-1)[:nf] < 0, 1] |= 0x80
    return out, errors, (g + nf) % 8
