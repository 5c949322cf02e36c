"""The data path of the IEEE 802.11a/g OFDM PHY (clause 17; 802.11p / j at half and quarter clock) around the K = 7, R = 1/2 decode, as
vit_hip_wifi_deinterleave_batch, vit_hip_wifi_signal_batch and vit_hip_wifi_data_batch run it (include/vit_hip.h): the rate table, the
interleaver's map, the rules of the three calls on the host (wifi_deinterleave_numpy, wifi_signal_parse_numpy, wifi_descramble_numpy),
the transmit side for tests (wifi_signal_field_numpy, wifi_ppdu_numpy) and WifiDecoder, the six calls from the demapper's soft bits to
PSDU octets with their FCS syndrome.  The GPU side is BatchDecoder.wifi_deinterleave / wifi_signal_parse / wifi_descramble (decoder.py).
Out of scope: synchronisation, channel estimation and demapping; 802.11n/ac and 802.11b; bucketing frames by length; a transmitter on
the card; A-MPDU delimiters."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from .synth import encode_bits_numpy

# g0 = 133, g1 = 171 (octal) in the package's convention -- bit k of a polynomial taps the input bit of k steps ago --, in the order
# (A, B): A[n] = x[n]^x[n-2]^x[n-3]^x[n-5]^x[n-6], B[n] = x[n]^x[n-1]^x[n-2]^x[n-3]^x[n-6].  The stock Voyager code
WIFI_POLYNOMIALS = (109, 79)
WIFI_SIGNAL_STEPS = 24
WIFI_MAX_LENGTH = 4095


@dataclass(frozen=True)
class WifiRate:
    """one row of the rate table: Mbit/s at 20 MHz, coded bits per subcarrier, code rate (numerator, denominator), coded and data bits
    per OFDM symbol, the SIGNAL field's R1 R2 R3 R4"""
    mbps: int
    n_bpsc: int
    code_rate: tuple
    n_cbps: int
    n_dbps: int
    signal_bits: tuple

    @property
    def s(self) -> int:
        return max(self.n_bpsc // 2, 1)


WIFI_RATES = (
    WifiRate(6, 1, (1, 2), 48, 24, (1, 1, 0, 1)), WifiRate(9, 1, (3, 4), 48, 36, (1, 1, 1, 1)),
    WifiRate(12, 2, (1, 2), 96, 48, (0, 1, 0, 1)), WifiRate(18, 2, (3, 4), 96, 72, (0, 1, 1, 1)),
    WifiRate(24, 4, (1, 2), 192, 96, (1, 0, 0, 1)), WifiRate(36, 4, (3, 4), 192, 144, (1, 0, 1, 1)),
    WifiRate(48, 6, (2, 3), 288, 192, (0, 0, 0, 1)), WifiRate(54, 6, (3, 4), 288, 216, (0, 0, 1, 1)),
)
# which of the mother code's bits one puncturing period sends, in the order A1 B1 A2 B2 ...
_KEEP = {(1, 2): (1, 1), (2, 3): (1, 1, 1, 0), (3, 4): (1, 1, 1, 0, 0, 1)}


def _rate(rate) -> WifiRate:
    if not 0 <= int(rate) <= 7:
        raise ValueError("rate must be 0 .. 7")
    return WIFI_RATES[int(rate)]


def wifi_interleave_map(rate: int):
    """j[k], k in [0, N_CBPS): the place in the transmitted OFDM symbol of coded bit k.  int32 [N_CBPS], a permutation"""
    r = _rate(rate)
    k = np.arange(r.n_cbps)
    i = (r.n_cbps // 16) * (k % 16) + k // 16
    return (r.s * (i // r.s) + (i + r.n_cbps - 16 * i // r.n_cbps) % r.s).astype(np.int32)


def _source_index(rate: int, n_steps: int):
    """for every (step n, output o) of the first n_steps steps, the element of the frame it is, or -1 where nothing was sent.  [n_steps * 2]"""
    r = _rate(rate)
    keep = np.asarray(_KEEP[r.code_rate])
    q = np.arange(2 * n_steps)
    sent = keep[q % keep.size] != 0
    c = int(keep.sum()) * (q // keep.size) + (np.cumsum(keep) - 1)[q % keep.size]
    return np.where(sent, (c // r.n_cbps) * r.n_cbps + wifi_interleave_map(rate)[c % r.n_cbps], -1)


def wifi_deinterleave_numpy(soft, max_sym: int, S: int, rate=0, n_sym=None, n_steps=None):
    """the rule of vit_hip_wifi_deinterleave_batch on the host: soft [frames][>= max_sym * N_CBPS] -> [frames][S][2] of its dtype.
    rate, n_sym, n_steps: scalars or one per frame (n_sym None: max_sym; n_steps None: n_sym * N_DBPS); a rate above 7 erases the frame"""
    soft = np.asarray(soft)
    if soft.ndim != 2:
        raise ValueError("soft must be [frames][elements]")
    frames, max_sym, S = soft.shape[0], int(max_sym), int(S)
    if max_sym < 1 or S < 1:
        raise ValueError("max_sym and S must be at least 1")
    rates = np.broadcast_to(np.asarray(rate, dtype=np.int64), (frames,))
    syms = np.broadcast_to(np.asarray(max_sym if n_sym is None else n_sym, dtype=np.int64), (frames,))
    steps = None if n_steps is None else np.broadcast_to(np.asarray(n_steps, dtype=np.int64), (frames,))
    out = np.zeros((frames, 2 * S), dtype=soft.dtype)
    for f in range(frames):
        if not 0 <= rates[f] <= 7:
            continue
        r = WIFI_RATES[rates[f]]
        if soft.shape[1] < max_sym * r.n_cbps:
            raise ValueError(f"frame {f} needs {max_sym * r.n_cbps} soft bits")
        lim = min(int(syms[f]), max_sym) * r.n_dbps
        n = min(lim if steps is None else int(steps[f]), lim, S)
        src = _source_index(int(rates[f]), n)
        out[f, :2 * n] = np.where(src >= 0, soft[f][np.maximum(src, 0)], 0)
    return out.reshape(frames, S, 2)


def wifi_signal_parse_numpy(bytes3):
    """the rule of vit_hip_wifi_signal_batch on the host: the 3 decoded bytes of every SIGNAL field, uint8 [frames][>= 3] -> uint32
    [frames][5] = (rate_index, length, n_sym, n_steps, valid)"""
    b = np.asarray(bytes3, dtype=np.uint8)
    if b.ndim != 2 or b.shape[1] < 3:
        raise ValueError("bytes must be [frames][>= 3]")
    bits = np.unpackbits(b[:, :3], axis=1).astype(np.int64)
    out = np.zeros((b.shape[0], 5), dtype=np.uint32)
    patterns = {r.signal_bits: m for m, r in enumerate(WIFI_RATES)}
    for f in range(b.shape[0]):
        m = patterns.get(tuple(bits[f, :4].tolist()), 8)
        length = int((bits[f, 5:17] << np.arange(12)).sum())
        valid = m < 8 and bits[f, :18].sum() % 2 == 0 and bits[f, 4] == 0 and length >= 1
        n_steps = 16 + 8 * length + 6 if valid else 0
        n_sym = -(-n_steps // WIFI_RATES[m].n_dbps) if valid else 0
        out[f] = (m, length, n_sym, n_steps, int(valid))
    return out


def wifi_scrambler_numpy(seed: int, n: int):
    """the first n bits of the sequence whose first seven are `seed` (p[0] in the highest of its 7 bits): p[t] = p[t-4] ^ p[t-7]"""
    p = np.zeros(max(int(n), 7), dtype=np.uint8)
    p[:7] = (int(seed) >> np.arange(6, -1, -1)) & 1
    for t in range(7, p.size):
        p[t] = p[t - 4] ^ p[t - 7]
    return p[:int(n)]


def wifi_descramble_numpy(bytes, S: int, lengths, max_length: int = WIFI_MAX_LENGTH):
    """the rule of vit_hip_wifi_data_batch on the host: the decoded bytes of every DATA field, uint8 [frames][>= ceil((S - 6) / 8)], and
    one LENGTH per frame -> (psdu, status): psdu a list of uint8 arrays, frame f's len_f octets, status uint32 [frames][4] =
    (length_used, seed, service, fcs_syndrome)"""
    b = np.asarray(bytes, dtype=np.uint8)
    n_bits = int(S) - 6
    if b.ndim != 2 or n_bits < 16 or b.shape[1] < (n_bits + 7) // 8:
        raise ValueError("bytes must be [frames][>= ceil((S - 6) / 8)], S at least 22")
    lengths = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (b.shape[0],))
    psdu, status = [], np.zeros((b.shape[0], 4), dtype=np.uint32)
    for f in range(b.shape[0]):
        d = np.unpackbits(b[f])[:n_bits]
        seed = int((d[:7].astype(np.int64) << np.arange(6, -1, -1)).sum())
        u = d ^ wifi_scrambler_numpy(seed, n_bits)
        n = min(int(lengths[f]), int(max_length), (n_bits - 16) // 8)
        octets = np.packbits(u[16:16 + 8 * n].reshape(n, 8), axis=1, bitorder="little").reshape(-1)
        syndrome = 0xFFFFFFFF
        if n >= 4:
            syndrome = zlib.crc32(octets[:n - 4].tobytes()) ^ int.from_bytes(octets[n - 4:].tobytes(), "little")
        psdu.append(octets)
        status[f] = (n, seed, int((u[:16].astype(np.int64) << np.arange(16)).sum()), syndrome)
    return psdu, status


def _soft(bits, amplitude, dtype):
    return np.where(np.asarray(bits) != 0, amplitude, -amplitude).astype(dtype)


def _interleave(coded, rate):
    """coded bits [n_sym * N_CBPS] -> transmit order, symbol by symbol"""
    r = _rate(rate)
    out = np.empty_like(coded).reshape(-1, r.n_cbps)
    out[:, wifi_interleave_map(rate)] = coded.reshape(-1, r.n_cbps)
    return out.reshape(-1)


def wifi_signal_field_numpy(rate: int, length: int, amplitude: int = 127, dtype=np.int16):
    """the SIGNAL field on the transmit side: RATE, reserved, LENGTH (LSB first), parity and six tail bits, encoded at rate 1/2 and
    interleaved as one BPSK symbol -> 48 soft bits of +-amplitude"""
    r = _rate(rate)
    if not 0 <= int(length) <= WIFI_MAX_LENGTH:
        raise ValueError("length must be 0 .. 4095")
    bits = np.zeros(18, dtype=np.uint8)
    bits[:4] = r.signal_bits
    bits[5:17] = (int(length) >> np.arange(12)) & 1
    bits[17] = bits[:17].sum() % 2
    coded = encode_bits_numpy(7, 2, WIFI_POLYNOMIALS, np.packbits(np.concatenate([bits, np.zeros(6, dtype=np.uint8)])))[0, :24].reshape(-1)
    return _soft(_interleave(coded, 0), amplitude, dtype)


def wifi_ppdu_numpy(psdu, rate: int, seed: int, amplitude: int = 127, dtype=np.int16):
    """the DATA field on the transmit side: SERVICE (16 zero bits) + PSDU octets LSB first + six tail bits + pad bits to whole OFDM
    symbols, scrambled from the state whose first seven output bits are `seed` (1 .. 127), the tail bits zeroed, encoded, punctured
    and interleaved -> n_sym * N_CBPS soft bits of +-amplitude"""
    r = _rate(rate)
    psdu = np.asarray(psdu, dtype=np.uint8).reshape(-1)
    if not 1 <= int(seed) <= 127:
        raise ValueError("seed must be 1 .. 127")
    n_steps = 16 + 8 * psdu.size + 6
    n_sym = -(-n_steps // r.n_dbps)
    data = np.zeros(n_sym * r.n_dbps, dtype=np.uint8)
    data[16:16 + 8 * psdu.size] = np.unpackbits(psdu, bitorder="little")
    data ^= wifi_scrambler_numpy(seed, data.size)
    data[n_steps - 6:n_steps] = 0
    x = np.concatenate([np.zeros(6, dtype=np.uint8), data])
    coded = np.zeros((data.size, 2), dtype=np.uint8)
    for o, g in enumerate(WIFI_POLYNOMIALS):
        for k in range(7):
            if (g >> k) & 1:
                coded[:, o] ^= x[6 - k:6 - k + data.size]
    keep = np.asarray(_KEEP[r.code_rate])
    sent = coded.reshape(-1)[np.tile(keep, 2 * data.size // keep.size) != 0]
    return _soft(_interleave(sent, rate), amplitude, dtype)


class WifiDecoder:
    """the receive side on the card, from the demapper's soft bits of many PPDUs to PSDU octets: SIGNAL de-interleave, decode, parse, DATA
    de-interleave at every frame's own rate and length, decode, descramble and check -- six launches, no host synchronisation.
    dec_signal, dec_data: BatchDecoders of WIFI_POLYNOMIALS on one device (two, as a decoder keeps one workspace per length; they may be
    the same object).  Buffers are sized for max_sym OFDM symbols at 54 Mbit/s and allocated once."""

    def __init__(self, dec_signal, dec_data, max_sym: int):
        max_sym = int(max_sym)
        if max_sym < 1:
            raise ValueError("max_sym must be at least 1")
        for d in (dec_signal, dec_data):
            if (d.K, d.R) != (7, 2):
                raise ValueError("WifiDecoder needs K = 7, R = 1/2 decoders of WIFI_POLYNOMIALS")
        self.dec_signal, self.dec_data, self.max_sym = dec_signal, dec_data, max_sym
        self.S = max_sym * 216
        self.max_length = min((self.S - 22) // 8, WIFI_MAX_LENGTH)
        self._frames = -1

    def _buffers(self, frames):
        if frames != self._frames:
            d, t = self.dec_data, self.dec_data.torch
            self._sig_sym = d._empty((frames, WIFI_SIGNAL_STEPS, 2), d._soft_dtype)
            self._sig_bytes = d._empty((frames, 3), t.uint8)
            self._sym = d._empty((frames, self.S, 2), d._soft_dtype)
            self._bytes = d._empty((frames, (self.S - 6 + 7) // 8), t.uint8)
            self._frames = frames
        return self._sig_sym, self._sig_bytes, self._sym, self._bytes

    def decode(self, signal_soft, data_soft, out=None):
        """signal_soft [frames][48], data_soft [frames][max_sym * 288] (frame f's n_sym * N_CBPS soft bits first), CUDA tensors of the
        decoders' symbol dtype.  returns (psdu uint8 [frames][max_length], status int32 [frames][4], signal int32 [frames][5]) as device
        tensors holding the uint32 values of the ABI; octets at or behind a frame's length_used are not written.  out = the same three
        reuses those tensors"""
        ds, dd = self.dec_signal, self.dec_data
        t = dd.torch
        frames = int(signal_soft.shape[0])
        sig_sym, sig_bytes, sym, dbytes = self._buffers(frames)
        if out is None:
            out = (dd._empty((frames, self.max_length), t.uint8), dd._empty((frames, 4), t.int32), dd._empty((frames, 5), t.int32))
        psdu, status, signal = out
        ds.wifi_deinterleave(signal_soft, 1, WIFI_SIGNAL_STEPS, rate=0, out=sig_sym)
        ds.decode(sig_sym, WIFI_SIGNAL_STEPS - 6, out=sig_bytes)
        ds.wifi_signal_parse(sig_bytes, out=signal)
        dd.wifi_deinterleave(data_soft, self.max_sym, self.S, signal=signal, out=sym)
        dd.decode(sym, self.S - 6, out=dbytes)
        dd.wifi_descramble(dbytes, self.S, signal, max_length=self.max_length, out=(psdu, status))
        return psdu, status, signal
