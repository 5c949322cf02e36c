"""An independent restatement of the DVB-S outer stages for the tests: no index arithmetic.  The interleaver and the de-interleaver are
per-branch FIFOs stepped byte by byte behind a commutator, as EN 300 421 draws them; the energy-dispersal sequence is a 15-stage shift
register clocked bit by bit through a group of eight packets, its output gated off under the seven upright sync bytes.  Never imports
the code under test."""
from collections import deque

import numpy as np


class DelayLines:
    """B branches behind a commutator; branch j is a FIFO of cells[j] bytes filled with zeros (0: a wire)"""

    def __init__(self, cells):
        self.lines = [deque([0] * c) for c in cells]
        self.at = 0

    def step(self, byte):
        line = self.lines[self.at]
        self.at = (self.at + 1) % len(self.lines)
        if not line:
            return byte
        line.append(byte)
        return line.popleft()

    def run(self, data):
        return np.array([self.step(int(b)) for b in np.asarray(data, dtype=np.uint8).reshape(-1)], dtype=np.uint8)


def interleave(packets, B, M):
    """the transmitter: branch j delays by j M bytes of its own; the delay lines start with zeros"""
    x = np.asarray(packets, dtype=np.uint8)
    return DelayLines([j * M for j in range(B)]).run(x).reshape(x.shape)


def history_packets(B, M, n):
    longest, H = (B - 1) * M * B, 0
    while H * n < longest:
        H += 1
    return H


def deinterleave(packets, B, M, hist=None, fill=0):
    """the receiver, one row: the real history packets, then `packets`, go through delay lines of (B-1-j) M bytes that start with
    zeros; the first H packets that come out still hold some of those zeros and are dropped.  returns (out [max(0, T-H)][n], the new
    history [H][n] with zeros in front of the real packets, the new fill)"""
    x = np.asarray(packets, dtype=np.uint8)
    n = x.shape[1]
    H = history_packets(B, M, n)
    fill = min(int(fill), H) if hist is not None else 0
    real = [np.asarray(hist, dtype=np.uint8).reshape(H, n)[H - fill:]] if fill else []
    S = np.concatenate(real + [x])
    y = DelayLines([(B - 1 - j) * M for j in range(B)]).run(S).reshape(S.shape)
    keep = min(H, S.shape[0])
    new = np.zeros((H, n), dtype=np.uint8)
    if keep:
        new[H - keep:] = S[S.shape[0] - keep:]
    return y[H:], new, keep


class Prbs:
    """1 + x^14 + x^15"""

    def __init__(self):
        self.reg = [int(c) for c in "100101010000000"]

    def bit(self):
        out = self.reg[13] ^ self.reg[14]
        self.reg = [out] + self.reg[:14]
        return out

    def byte(self):
        v = 0
        for _ in range(8):
            v = (v << 1) | self.bit()
        return v


def sequence_bytes(count):
    p = Prbs()
    return [p.byte() for _ in range(count)]


def scramble(packets, phase):
    """transport packets [N][188] whose packet 0 is packet `phase` of a group of eight -> the same, scrambled or descrambled: the
    register is loaded behind the sync byte that heads a group, which is inverted, and is clocked through every byte up to the next
    one; under a sync byte its output is gated off"""
    x = np.asarray(packets, dtype=np.uint8)
    out = x.copy()
    prbs = Prbs()
    for _ in range(188 * int(phase) - 1):                         # loaded behind the group's first sync byte, clocked through every
        prbs.byte()                                               # byte since: the register as it stands in front of packet `phase`
    for f in range(x.shape[0]):
        head = (int(phase) + f) % 8 == 0
        for i in range(188):
            if i == 0:
                if head:
                    prbs = Prbs()
                    out[f, 0] ^= 0xFF
                else:
                    prbs.byte()                                   # runs on, gated
            else:
                out[f, i] ^= prbs.byte()
    return out


def bits_of(v):
    return bin(int(v)).count("1")


def vote(sync_bytes):
    """the group phase 0 .. 7 of the first packet that leaves the fewest wrong sync bits; the lower on a tie; 8 without a packet"""
    best, best_cost = 8, None
    for g in range(8):
        cost = sum(bits_of(int(s) ^ (0xB8 if (g + f) % 8 == 0 else 0x47)) for f, s in enumerate(sync_bytes))
        if len(sync_bytes) and (best_cost is None or cost < best_cost):
            best, best_cost = g, cost
    return best


def derandomize(packets, phase=None, rs_status=None):
    """one row, all packets: (out [N][188], sync bit errors [N], next phase or 0xFFFFFFFF)"""
    x = np.asarray(packets, dtype=np.uint8)[:, :188]
    g = 8 if phase is None or not 0 <= int(phase) < 8 else int(phase)
    if g == 8:
        g = vote(x[:, 0].tolist())
    if g == 8:
        return x[:0].copy(), np.zeros(0, dtype=np.int64), 0xFFFFFFFF
    out = scramble(x, g)
    errors = np.array([bits_of(int(x[f, 0]) ^ (0xB8 if (g + f) % 8 == 0 else 0x47)) for f in range(x.shape[0])], dtype=np.int64)
    if rs_status is not None:
        for f in range(x.shape[0]):
            if int(rs_status[f]) < 0:
                out[f, 1] |= 0x80
    return out, errors, (g + x.shape[0]) % 8
