"""The IS-95A forward traffic channel, rate set 1, around the K = 9, R = 1/2 decode, as vit_hip_is95_deinterleave_batch and
vit_hip_is95_rate_decide_batch run it (include/vit_hip.h): the frame formats, the block interleaver, the rules of the two calls on the host
(is95_deinterleave_numpy, is95_rate_decide_numpy), the transmit side for tests (is95_traffic_frame_numpy) and Is95TrafficDecoder, the
nine calls from Walsh-despread soft symbols to info bits and a rate per frame.  The GPU side is BatchDecoder.is95_deinterleave /
is95_channel_errors / is95_rate_decide (decoder.py).  The constants are written from memory of TIA/EIA-95 7.1.3; include/vit_hip.h states the rule.
Out of scope: rate set 2 (14400 and its puncturing); the long-code generator itself (the caller supplies the decimated bits);
power-control bit extraction; sync and paging channels (continuous encoding: decode_stream); the reverse link (other interleaver, 64-ary
orthogonal modulation); cdma2000 radio configurations 3 and up (R = 1/4 with puncturing); any rate-decision policy beyond the rule."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .crc import CRCCode, crc_append_numpy
from .synth import encode_bits_numpy

# The standard's generators 753 and 561 (octal) read with the leftmost bit of 753 on the encoder INPUT -- as 133 / 171 are read for 802.11
# (wifi.WIFI_POLYNOMIALS) -- in the package's convention, where bit k of a polynomial taps the input bit of k steps ago: 0o657, 0o435, the
# bit reversals of the stock code "CDMA IS-95A" (491, 369) = 0o753, 0o561, which is the literal reading under that convention.  Nothing in
# this module depends on the polynomials (the calls need R = 2 alone); both sets run through it: the stock one on its specialised kernels,
# this one on the GENERIC K = 9 kernels.
IS95_POLYNOMIALS = (431, 285)
IS95_CRC12 = CRCCode(12, 0xF13, 0xFFF, 0)             # the frame quality indicator of a 9600 bit/s frame, over its 172 info bits
IS95_CRC8 = CRCCode(8, 0x9B, 0xFF, 0)                 # ... of a 4800 bit/s frame, over its 80 info bits
IS95_SYMBOLS = 384
IS95_INFO_BYTES = 22
IS95_ERASED = 4


@dataclass(frozen=True)
class Is95Rate:
    """one frame format of rate set 1: bit/s, the repetition of a code symbol, info bits, the CRC behind them (None: none), the bits in
    front of the 8 tail bits"""
    bps: int
    repeat: int
    info_bits: int
    crc: CRCCode
    L: int

    @property
    def steps(self) -> int:
        return self.L + 8

    @property
    def n_bytes(self) -> int:
        return self.L // 8


IS95_RATE_SET_1 = (Is95Rate(9600, 1, 172, IS95_CRC12, 184), Is95Rate(4800, 2, 80, IS95_CRC8, 88), Is95Rate(2400, 4, 40, None, 40),
                   Is95Rate(1200, 8, 16, None, 16))


def is95_permutation():
    """A[i], i in [0, 384): received symbol i is symbol A(i) = 64 (i mod 6) + BRO6(i div 6) of the repeated stream.  int32 [384]"""
    i = np.arange(IS95_SYMBOLS)
    c = i // 6
    bro = sum(((c >> b) & 1) << (5 - b) for b in range(6))
    return (64 * (i % 6) + bro).astype(np.int32)


def _mask_bits(scramble, frames):
    """None, or the scramble bits [frames][384] of packed bytes [48] (one mask) or [frames][48]"""
    if scramble is None:
        return None
    s = np.asarray(scramble, dtype=np.uint8)
    if s.ndim == 1:
        s = np.broadcast_to(s, (frames, s.size))
    if s.shape != (frames, IS95_SYMBOLS // 8):
        raise ValueError("scramble must be 48 packed bytes, or [frames][48]")
    return np.unpackbits(s, axis=1)


def is95_deinterleave_numpy(symbols, scramble=None, shift: int = 0, clamp_lo: int = None, clamp_hi: int = None):
    """the rule of vit_hip_is95_deinterleave_batch on the host: symbols [frames][384], int8 or int16 -> the four arrays [frames][S_h][2] of
    its dtype.  scramble: the mask packed MSB-first, uint8 [48] for the whole batch or [frames][48] (None: off); sums and the negation are
    int32; the clamp defaults to the range of the dtype"""
    x = np.asarray(symbols)
    if x.ndim != 2 or x.shape[1] != IS95_SYMBOLS or x.dtype not in (np.int8, np.int16):
        raise ValueError("symbols must be an int8 or int16 array [frames][384]")
    info = np.iinfo(x.dtype)
    lo, hi, shift = (info.min if clamp_lo is None else int(clamp_lo)), (info.max if clamp_hi is None else int(clamp_hi)), int(shift)
    if not 0 <= shift <= 15 or not info.min <= lo <= hi <= info.max:
        raise ValueError("shift must be 0 .. 15, the clamp a range of the dtype")
    v = x.astype(np.int64)
    bits = _mask_bits(scramble, x.shape[0])
    if bits is not None:
        v = np.where(bits != 0, -v, v)
    s = np.empty_like(v)
    s[:, is95_permutation()] = v                                                   # y[i] = s[A(i)]
    out = []
    for h, r in enumerate(IS95_RATE_SET_1):
        acc = s.reshape(x.shape[0], IS95_SYMBOLS // r.repeat, r.repeat).sum(axis=2)
        acc = (acc + ((1 << shift) >> 1)).astype(np.int32) >> shift
        out.append(np.clip(acc, lo, hi).astype(x.dtype).reshape(x.shape[0], r.steps, 2))
    return tuple(out)


def is95_rate_decide_numpy(bytes, errors, compared, syndrome, max_ser_num, ser_den: int):
    """the rule of vit_hip_is95_rate_decide_batch on the host.  bytes: four uint8 arrays [frames][>= 23 / 11 / 5 / 2], None for an absent
    hypothesis; errors, compared: four arrays [frames] (those of absent hypotheses are not read); syndrome: two arrays [frames];
    max_ser_num: four ints.  returns (decision uint32 [frames][4] = (rate, info_bits, errors, compared), info uint8 [frames][22])"""
    present = [b is not None for b in bytes]
    if len(bytes) != 4 or not any(present) or int(ser_den) < 1:
        raise ValueError("four hypotheses, not all absent; ser_den at least 1")
    frames = next(np.asarray(b).shape[0] for b in bytes if b is not None)
    decision = np.zeros((frames, 4), dtype=np.uint32)
    info = np.zeros((frames, IS95_INFO_BYTES), dtype=np.uint8)
    for f in range(frames):
        best = None
        for h in range(4):
            if not present[h] or (h < 2 and int(syndrome[h][f]) & 0xFFFFFFFF):
                continue
            e, c = int(errors[h][f]) & 0xFFFFFFFF, int(compared[h][f]) & 0xFFFFFFFF
            if c == 0 or e * int(ser_den) > c * int(max_ser_num[h]):
                continue
            if best is None or e * best[2] < best[1] * c:
                best = (h, e, c)
        if best is None:
            decision[f, 0] = IS95_ERASED
            continue
        n = IS95_RATE_SET_1[best[0]].info_bits
        decision[f] = (best[0], n, best[1], best[2])
        got = np.unpackbits(np.asarray(bytes[best[0]][f], dtype=np.uint8))[:n]
        info[f] = np.packbits(np.concatenate([got, np.zeros(8 * IS95_INFO_BYTES - n, dtype=np.uint8)]))
    return decision, info


def is95_traffic_frame_numpy(info_bits, h: int, scramble=None, polynomials=IS95_POLYNOMIALS, amplitude: int = 127, dtype=np.int16):
    """the transmit side, for tests: the info bits of one frame (0 / 1, 172, 80, 40 or 16 of them by h) -> (symbols [384] of +-amplitude as
    received without noise, frame bytes uint8 [L_h / 8]: info bits, CRC, in front of the tail).  CRC MSB-first, 8 zero tail bits, the
    package's encoder, every symbol repeated 2^h times, interleaved, negated where its scramble bit (48 packed bytes, MSB-first) is 1"""
    if not 0 <= int(h) <= 3:
        raise ValueError("h must be 0 .. 3")
    r = IS95_RATE_SET_1[int(h)]
    bits = np.asarray(info_bits, dtype=np.uint8).reshape(-1)
    if bits.size != r.info_bits or (bits > 1).any():
        raise ValueError(f"hypothesis {h} carries {r.info_bits} info bits")
    frame = np.packbits(np.concatenate([bits, np.zeros(r.L - r.info_bits, dtype=np.uint8)]))
    if r.crc is not None:
        frame = crc_append_numpy(r.crc, frame, r.info_bits)
    coded = encode_bits_numpy(9, 2, polynomials, frame)[0].reshape(-1)            # [S_h][2] -> c[2 n + o]
    s = np.repeat(coded, r.repeat)
    y = np.where(s[is95_permutation()] != 0, int(amplitude), -int(amplitude)).astype(np.int64)
    mask = _mask_bits(scramble, 1)
    if mask is not None:
        y = np.where(mask[0] != 0, -y, y)
    return y.astype(dtype), frame


def _decode(dec, symbols, L, workspace, out):
    """BatchDecoder.decode (vit_hip_decode_batch) of dense symbols [frames][L + 8][2] into `out`, in a workspace of the caller's --
    dec.new_workspace(frames, L) -- instead of the decoder's own, which another user of the decoder may grow and move"""
    import ctypes as C

    from . import _lib
    frames = dec._check_symbols(symbols, L + dec.K - 1)
    at = lambda x: C.c_void_p(x.data_ptr())
    _lib.check(_lib.load().vit_hip_decode_batch(dec._handle._h, at(symbols), frames, L, at(workspace), workspace.numel(), at(out), None, None, None,
                                                dec._stream()))
    return out


class Is95TrafficDecoder:
    """the receive side on the card, from Walsh-despread soft symbols of many forward traffic frames to info bits and a rate per frame: one
    de-interleave, four decodes, two crc_check, the four error counts in one is95_channel_errors and one rate decision -- nine calls, no
    host synchronisation, no memset, capturable as one graph once the buffers stand (they are allocated at the first push of a frame
    count, the four decision workspaces too).  Four channel_errors calls give the same counts eagerly; their eight memset nodes do
    not survive the replay of a graph on every runtime (include/vit_hip.h).  dec: a BatchDecoder of K = 9, R = 1/2 -- the stock code or IS95_POLYNOMIALS.  max_ser = ((n0, n1, n2, n3),
    den): hypothesis h passes only with errors * den <= compared * n_h.  shift, clamp: those of is95_deinterleave (clamp None: the decoder's
    soft_decision_low / high)."""

    def __init__(self, dec, max_ser=((1, 1, 1, 1), 4), shift: int = 0, clamp=None):
        if (dec.K, dec.R) != (9, 2):
            raise ValueError("Is95TrafficDecoder needs a K = 9, R = 1/2 decoder")
        num, den = max_ser
        if len(num) != 4 or int(den) < 1 or min(int(n) for n in num) < 0:
            raise ValueError("max_ser must be ((n0, n1, n2, n3), den) with den at least 1")
        i = dec._handle.info
        self.dec, self.max_ser, self.shift = dec, (tuple(int(n) for n in num), int(den)), int(shift)
        self.clamp = (i.soft_decision_low, i.soft_decision_high) if clamp is None else (int(clamp[0]), int(clamp[1]))
        self._frames = -1

    def _buffers(self, frames):
        if frames != self._frames:
            d, t = self.dec, self.dec.torch
            self._sym = tuple(d._empty((frames, r.steps, 2), d._soft_dtype) for r in IS95_RATE_SET_1)
            self._bytes = tuple(d._empty((frames, r.n_bytes), t.uint8) for r in IS95_RATE_SET_1)
            self._ws = tuple(d.new_workspace(frames, r.L) for r in IS95_RATE_SET_1)
            self._counts = tuple((d._empty((frames,), t.int32), d._empty((frames,), t.int32)) for _ in IS95_RATE_SET_1)
            self._syndrome = tuple(d._empty((frames,), t.int32) for _ in range(2))
            self._crc = tuple(d._empty((frames,), t.int32) for _ in range(2))
            self._frames = frames
        return self._sym, self._bytes, self._ws, self._counts, self._syndrome

    def push(self, symbols, scramble=None, out=None):
        """symbols: [frames][384] of the decoder's symbol dtype on its device (rows may be wider apart); scramble: None, uint8 [48] or
        [frames][48].  returns (decisions int32 [frames][4] = (rate, info_bits, errors, compared), the uint32 values of the ABI, rate 4
        for an erased frame; info uint8 [frames][22]); out = the same two reuses those tensors"""
        d, t = self.dec, self.dec.torch
        frames = int(symbols.shape[0])
        sym, dbytes, ws, counts, syndrome = self._buffers(frames)
        if out is None:
            out = (d._empty((frames, 4), t.int32), d._empty((frames, IS95_INFO_BYTES), t.uint8))
        d.is95_deinterleave(symbols, scramble=scramble, shift=self.shift, clamp=self.clamp, out=sym)
        for h, r in enumerate(IS95_RATE_SET_1):
            _decode(d, sym[h], r.L, ws[h], dbytes[h])
            if r.crc is not None:
                d.crc_check(r.crc, dbytes[h], r.info_bits, crc_out=self._crc[h], syndrome_out=syndrome[h])
        errors, compared = d.is95_channel_errors(sym, dbytes, out=([c[0] for c in counts], [c[1] for c in counts]))
        return d.is95_rate_decide(dbytes, errors, compared, syndrome, self.max_ser[0], self.max_ser[1], out=out)
