"""The front of the DVB-T receive chain (ETSI EN 300 744 clauses 4.3.3 and 4.3.4) as vit_hip_dvbt_deinterleave_batch runs it
(include/vit_hip.h): the modes and rates, the symbol permutation H, the rule of the call on the host (dvbt_deinterleave_numpy), the
transmit side for tests (dvbt_puncture_numpy, dvbt_interleave_numpy) and DvbtDecoder, the receiver from the demapper's soft bits to
transport packets: inner de-interleave + depuncture -> stream decode -> the DVB-S outer chain (sync byte, Forney (12, 17), RS(204,188),
energy dispersal).  The GPU side is BatchDecoder.dvbt_deinterleave (decoder.py).
The stock code COMMON_CODES[2].G = (109, 79) is (133, 171) octal = (Y, X): X is output index 1 of a trellis step, Y index 0.
Out of scope: hierarchical modes, the DVB-H in-depth interleaver, OFDM demodulation, pilots, TPS decoding and demapping, DVB-T2, a
transmitter on the card."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class DvbtMode:
    """one transmission mode: its index in the ABI, Mmax, the data carriers Nmax of an OFDM symbol, Nr, the bits of R' that are XORed
    into its new bit and the positions bits Nr-2 .. 0 of R' take in R"""
    index: int
    m_max: int
    n_max: int
    n_r: int
    taps: tuple
    wires: tuple


DVBT_MODES = {
    "2k": DvbtMode(0, 2048, 1512, 11, (0, 3), (0, 7, 5, 1, 8, 2, 6, 9, 3, 4)),
    "4k": DvbtMode(1, 4096, 3024, 12, (0, 2), (7, 10, 5, 8, 1, 2, 4, 9, 0, 3, 6)),
    "8k": DvbtMode(2, 8192, 6048, 13, (0, 1, 4, 6), (5, 11, 3, 0, 10, 8, 6, 9, 2, 4, 1, 7)),
}
# code rates by rate index, and what one puncturing period sends, in order: (output, step of the period); output 1 = X, 0 = Y
DVBT_RATES = ((1, 2), (2, 3), (3, 4), (5, 6), (7, 8))
_SENT = ("X1 Y1", "X1 Y1 Y2", "X1 Y1 Y2 X3", "X1 Y1 Y2 X3 Y4 X5", "X1 Y1 Y2 Y3 Y4 X5 Y6 X7")
DVBT_BIT_SHIFTS = (0, 63, 105, 42, 21, 84)


def _mode(mode) -> DvbtMode:
    if isinstance(mode, DvbtMode):
        return mode
    if mode not in DVBT_MODES:
        raise ValueError("mode must be '2k', '4k' or '8k'")
    return DVBT_MODES[mode]


def _check(v, rate):
    if int(v) not in (2, 4, 6):
        raise ValueError("v must be 2, 4 or 6")
    if not 0 <= int(rate) <= 4:
        raise ValueError("rate must be 0 .. 4")
    return int(v), int(rate)


@functools.lru_cache(maxsize=None)
def _permutation(name):
    m = DVBT_MODES[name]
    h, rp = [], 0
    for i in range(m.m_max):
        if i == 2:
            rp = 1
        elif i > 2:
            new = 0
            for b in m.taps:
                new ^= (rp >> b) & 1
            rp = (rp >> 1) | (new << (m.n_r - 2))
        r = 0
        for t, to in enumerate(m.wires):
            r |= ((rp >> (m.n_r - 2 - t)) & 1) << to
        hq = (i % 2) * (1 << (m.n_r - 1)) + r
        if hq < m.n_max:
            h.append(hq)
    h = np.array(h, dtype=np.int32)
    h.setflags(write=False)
    return h


def dvbt_symbol_permutation(mode):
    """H(q), q in [0, Nmax): int32, read-only, a permutation.  In an even OFDM symbol interleaver cell q is on carrier H(q), in an odd
    one on carrier H^-1(q)"""
    return _permutation(next(k for k, m in DVBT_MODES.items() if m is _mode(mode)))


def dvbt_steps_per_symbol(mode, v: int, rate: int) -> int:
    """trellis steps one OFDM symbol carries: Nmax v r"""
    v, rate = _check(v, rate)
    k, n = DVBT_RATES[rate]
    return _mode(mode).n_max * v // n * k


def _places(rate):
    """[k][2]: the place in the period's k + 1 sent bits of (step j, output o), or -1 where nothing is sent"""
    k = DVBT_RATES[rate][0]
    place = np.full((k, 2), -1, dtype=np.int64)
    for at, name in enumerate(_SENT[rate].split()):
        place[int(name[1:]) - 1, 1 if name[0] == "X" else 0] = at
    return place


def _source_index(mode, v, rate, odd):
    """for every (step n, output o) of one OFDM symbol, the element of the symbol [Nmax][v] it is, or -1 where nothing was sent"""
    m = _mode(mode)
    k = DVBT_RATES[rate][0]
    steps = dvbt_steps_per_symbol(m, v, rate)
    n = np.arange(steps)[:, None]
    place = _places(rate)[n % k, np.arange(2)[None, :]]
    di = (k + 1) * (n // k) + place
    word, r = di // v, di % v
    e = r // (v // 2) + 2 * (r % (v // 2))
    q = 126 * (word // 126) + (word % 126 - np.asarray(DVBT_BIT_SHIFTS)[e]) % 126
    h = dvbt_symbol_permutation(m)
    p = np.argsort(h) if odd else h
    return np.where(place >= 0, p[np.where(place >= 0, q, 0)] * v + e, -1).reshape(-1)


def dvbt_deinterleave_numpy(soft, mode, v: int, rate: int, parity=0):
    """the rule of vit_hip_dvbt_deinterleave_batch on the host: soft [rows][n_sym][Nmax * v] (or [n_sym][Nmax * v]: one row; cells in
    carrier order, v soft bits each) -> [rows][n_sym * steps][2] of its dtype, (Y, X) per trellis step, 0 where nothing was sent.
    parity: that of every row's first symbol, a scalar or one per row"""
    m = _mode(mode)
    v, rate = _check(v, rate)
    soft = np.asarray(soft)
    one = soft.ndim == 2
    soft = soft[None] if one else soft
    if soft.ndim != 3 or soft.shape[2] != m.n_max * v:
        raise ValueError("soft must be [rows][n_sym][Nmax * v]")
    rows, n_sym = soft.shape[:2]
    first = np.broadcast_to(np.asarray(parity, dtype=np.int64), (rows,))
    src = [_source_index(m, v, rate, odd) for odd in (0, 1)]
    out = np.zeros((rows, n_sym, src[0].size), dtype=soft.dtype)
    for r in range(rows):
        for y in range(n_sym):
            s = src[(int(first[r]) + y) & 1]
            out[r, y] = np.where(s >= 0, soft[r, y][np.maximum(s, 0)], 0)
    out = out.reshape(rows, -1, 2)
    return out[0] if one else out


def dvbt_puncture_numpy(coded, rate: int):
    """the transmit side: the mother code's output [steps][2] in the package's order (index 0 = Y, 1 = X), steps a multiple of the period
    -> the bits sent, in order, [steps (k + 1) / k]"""
    _, rate = _check(2, rate)
    coded = np.asarray(coded)
    k = DVBT_RATES[rate][0]
    if coded.ndim != 2 or coded.shape[1] != 2 or coded.shape[0] % k:
        raise ValueError("coded must be [steps][2] with whole puncturing periods")
    place = _places(rate).reshape(-1)
    order = np.argsort(np.where(place >= 0, place, 2 * k), kind="stable")[:k + 1]
    return coded.reshape(-1, 2 * k)[:, order].reshape(-1)


def dvbt_interleave_numpy(sent, mode, v: int, parity: int = 0):
    """the transmit side: the punctured bits of whole OFDM symbols [n_sym * Nmax * v] -> [n_sym][Nmax * v], cells in carrier order:
    demultiplexer, bit interleavers, symbol interleaver; parity is that of the first symbol"""
    m = _mode(mode)
    v, _ = _check(v, 0)
    sent = np.asarray(sent).reshape(-1)
    if sent.size % (m.n_max * v):
        raise ValueError("sent must hold whole OFDM symbols of Nmax * v bits")
    h = dvbt_symbol_permutation(m)
    out = np.empty((sent.size // (m.n_max * v), m.n_max, v), dtype=sent.dtype)
    w = np.arange(126)
    for y, x in enumerate(sent.reshape(-1, m.n_max, v)):
        cells = np.empty((m.n_max, v), dtype=sent.dtype)
        for r in range(v):
            e = r // (v // 2) + 2 * (r % (v // 2))
            cells[:, e] = x[:, r].reshape(-1, 126)[:, (w + DVBT_BIT_SHIFTS[e]) % 126].reshape(-1)
        if (int(parity) + y) & 1:
            out[y] = cells[h]
        else:
            out[y, h] = cells
    return out.reshape(out.shape[0], -1)


class DvbtDecoder:
    """the receive side on the card, from the demapper's soft bits to transport packets: BatchDecoder.dvbt_deinterleave, then a
    StreamDecoder (n_streams None) or MultiStreamDecoder configured as the DVB-S receiver -- marker=DVB_SYNC, period=1632, frames=True,
    rs=DVB_RS_204_188, deinterleave=DVB_INTERLEAVER, dvb_derandomize=True.  push(symbols) takes whole OFDM symbols, [n_sym][Nmax * v] (or
    [n_streams][n_sym][Nmax * v]; any trailing shape with that many elements) of the decoder's symbol dtype, in any number per push;
    the parity of the next symbol is a counter per stream on the device, ping-ponged between two tensors.  take_frames() returns what
    the receiver returns: (packets uint8 [k][188], sync_errors, rs_status) -- per stream with n_streams.  `rx` is the receiver itself."""

    def __init__(self, decoder, mode, v: int, rate: int, n_streams: int = None, window: int = None, parity: int = 0):
        from .frame_sync import DVB_SYNC
        from .dvb import DVB_INTERLEAVER
        from .reed_solomon import DVB_RS_204_188
        from .stream import MultiStreamDecoder, StreamDecoder
        if (decoder.K, decoder.R) != (7, 2):
            raise ValueError("DvbtDecoder needs a K = 7, R = 1/2 decoder of the stock polynomials (109, 79)")
        self.decoder, self.mode = decoder, _mode(mode)
        self.v, self.rate = _check(v, rate)
        self.n_streams = n_streams
        self.steps = dvbt_steps_per_symbol(self.mode, self.v, self.rate)
        kw = dict(marker=DVB_SYNC, period=1632, frames=True, rs=DVB_RS_204_188, deinterleave=DVB_INTERLEAVER, dvb_derandomize=True)
        self.rx = StreamDecoder(decoder, window, **kw) if n_streams is None else MultiStreamDecoder(decoder, int(n_streams), window, **kw)
        t = decoder.torch
        rows = 1 if n_streams is None else int(n_streams)
        self._parity = [t.full((rows,), int(parity), dtype=t.int32, device=decoder.device), t.zeros(rows, dtype=t.int32, device=decoder.device)]

    def _front(self, symbols):
        if symbols is None:
            return None
        rows = 1 if self.n_streams is None else self.n_streams
        cell = self.mode.n_max * self.v
        if symbols.numel() == 0 or symbols.numel() % (rows * cell) or (self.n_streams is not None and symbols.shape[0] != rows):
            raise ValueError("symbols must hold whole OFDM symbols of Nmax * v soft bits" + ("" if self.n_streams is None else " per stream"))
        out = self.decoder.dvbt_deinterleave(symbols.reshape(rows, -1, cell), self.mode, self.v, self.rate, parity=tuple(self._parity))
        self._parity.reverse()
        return out[0] if self.n_streams is None else out

    def push(self, symbols):
        return self.rx.push(self._front(symbols))

    def finish(self, symbols=None):
        return self.rx.finish(self._front(symbols))

    def take_frames(self):
        return self.rx.take_frames()
