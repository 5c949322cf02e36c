"""GSM channel decoding (3GPP TS 45.003) around the K = 5, R = 1/2 decode, as vit_hip_gsm_deinterleave_batch, vit_hip_gsm_fire_batch and
vit_hip_gsm_tchfs_batch run it (include/vit_hip.h): the burst interleavers, the Fire code of the control channels and the TCH/FS frame; the
rules of the three calls on the host (gsm_deinterleave_numpy, gsm_fire_numpy, gsm_tchfs_numpy), the transmit side for tests
(gsm_fire_encode_numpy, gsm_xcch_bursts_numpy, gsm_tchfs_bursts_numpy, gsm_facch_steal_numpy) and two receivers without a host
synchronisation, GsmControlDecoder and GsmTchfDecoder.  The GPU side is BatchDecoder.gsm_deinterleave / gsm_fire / gsm_tchfs (decoder.py).
The constants and maps are written from memory of TS 45.003 clauses 3.1, 4.1 and 4.3; include/vit_hip.h states the rule and the check values
of tests/test_gsm_cpu.py pin it.
Out of scope: GPRS CS-2..4 and EGPRS (puncturing tables, USF precoding); TCH/HS, EFR's preliminary CRC-8, AMR; SACCH/TCH multiframe
scheduling and deciphering (the caller negates with the A5 keystream); burst demodulation; per-row burst counts in one call; a transmitter
on the card."""
from __future__ import annotations

import numpy as np

from .crc import CRCCode, crc_numpy
from .synth import encode_bits_numpy

# G0 = 1 + D^3 + D^4, G1 = 1 + D + D^3 + D^4 in the package's convention, where bit k of a polynomial taps the input of k steps ago; not the
# stock "Basic K=5 R=1/2" (23, 25).  The GENERIC K = 5 kernels serve it.  Nothing in this module but the transmit side depends on it.
GSM_POLYNOMIALS = (25, 27)
GSM_BLOCK, GSM_DIAGONAL = 0, 1
GSM_BURST, GSM_CODED = 116, 456
GSM_FIRE_G = 0x10004820009                                # (D^23 + 1)(D^17 + D^3 + 1)
# the channels that need no kernel of their own, as codes for crc_check behind a plain decode
GSM_SCH_CRC10 = CRCCode(10, 0x175, 0, 0x3FF)              # SCH: 25 data bits, L = 35
GSM_RACH_CRC6 = CRCCode(6, 0x2F, 0, 0x3F)                 # RACH: 8 data bits; the syndrome is the BSIC the sender added
GSM_TCHFS_CRC3 = CRCCode(3, 0x3, 0, 0x7)                  # TCH/FS: over the first 50 class I bits


def _mode(mode):
    m = {"block": GSM_BLOCK, "diagonal": GSM_DIAGONAL}.get(mode, mode)
    if m not in (GSM_BLOCK, GSM_DIAGONAL):
        raise ValueError("mode must be GSM_BLOCK / 'block' or GSM_DIAGONAL / 'diagonal'")
    return m


def gsm_interleave_map(mode):
    """(burst, element), two int32 arrays [456]: coded bit k of block n is element[k] of the 116 of burst 4 n + burst[k]: j(k) = 2 ((49 k)
    mod 57) + ((k mod 8) div 4), behind the stealing flags at 57 and 58 where j >= 57; burst = k mod 4 (block) or k mod 8 (diagonal)"""
    k = np.arange(GSM_CODED)
    j = 2 * ((49 * k) % 57) + (k % 8) // 4
    return (k % (8 if _mode(mode) == GSM_DIAGONAL else 4)).astype(np.int32), np.where(j < 57, j, j + 2).astype(np.int32)


def gsm_deinterleave_numpy(bursts, mode, negate: bool = False, hist=None, fill=None):
    """the rule of vit_hip_gsm_deinterleave_batch on the host: bursts [rows][4 m][116], int8 or int16 -> (full [rows][m][228][2], class1
    [rows][m][189][2], class2 [rows][m][78], steal int32 [rows][m], n_out int32 [rows], hist_out [rows][4][116], fill_out int32 [rows]).
    hist [rows][4][116] and fill [rows] (4: the row has history) are what the call before returned; block mode takes none and returns
    None for the last two.  Slots behind a row's n_out are zeros"""
    x = np.asarray(bursts)
    mode = _mode(mode)
    if x.ndim != 3 or x.shape[2] != GSM_BURST or x.shape[1] % 4 or x.dtype not in (np.int8, np.int16):
        raise ValueError("bursts must be an int8 or int16 array [rows][4 m][116]")
    if mode == GSM_BLOCK and (hist is not None or fill is not None):
        raise ValueError("the block mode carries no history")
    if (hist is None) != (fill is None):
        raise ValueError("hist and fill come together")
    rows, m = x.shape[0], x.shape[1] // 4
    info = np.iinfo(x.dtype)
    sign = lambda v: np.minimum(-v.astype(np.int32), info.max) if negate else v.astype(np.int32)
    burst, element = gsm_interleave_map(mode)
    coded = np.zeros((rows, m, GSM_CODED), dtype=np.int32)
    steal = np.zeros((rows, m), dtype=np.int32)
    n_out = np.full(rows, m, dtype=np.int32)
    for r in range(rows):
        seq = sign(x[r])
        if mode == GSM_DIAGONAL:
            if hist is not None and int(np.asarray(fill)[r]) == 4:
                seq = np.concatenate([sign(np.asarray(hist)[r].reshape(4, GSM_BURST)), seq])
            else:
                n_out[r] = m - 1
        for n in range(n_out[r]):
            coded[r, n] = seq[4 * n + burst, element]
            if mode == GSM_DIAGONAL:
                steal[r, n] = seq[4 * n:4 * n + 4, 58].sum() + seq[4 * n + 4:4 * n + 8, 57].sum()
            else:
                steal[r, n] = seq[4 * n:4 * n + 4, 57:59].sum()
    coded = coded.astype(x.dtype)
    out = (coded.reshape(rows, m, 228, 2), coded[:, :, :378].reshape(rows, m, 189, 2).copy(), coded[:, :, 378:].copy(), steal, n_out)
    if mode == GSM_BLOCK:
        return out + (None, None)
    return out + (x[:, 4 * m - 4:].copy() if m else np.zeros((rows, 4, GSM_BURST), dtype=x.dtype), np.full(rows, 4, dtype=np.int32))


def _fire_remainder(bits):
    """r mod g of bits [...][n] (0 / 1, the coefficient of the highest power first), as Python ints in an object array [...]"""
    bits = np.asarray(bits)
    reg = np.zeros(bits.shape[:-1], dtype=object)
    for t in range(bits.shape[-1]):
        reg = reg * 2 + bits[..., t].astype(object)
        reg = np.where((reg >> 40) & 1, reg ^ GSM_FIRE_G, reg)
    return reg


def gsm_fire_encode_numpy(data):
    """the transmit side: data uint8 [...][23], d(8 i + b) bit 7 - b of byte i -> uint8 [...][28], the 40 parity bits behind them that
    make the remainder of the 224 bits mod g all ones"""
    data = np.asarray(data, dtype=np.uint8)
    if data.shape[-1] != 23:
        raise ValueError("data must be uint8 [...][23]")
    bits = np.concatenate([np.unpackbits(data, axis=-1), np.zeros(data.shape[:-1] + (40,), dtype=np.uint8)], axis=-1)
    parity = _fire_remainder(bits) ^ ((1 << 40) - 1)
    bits[..., 184:] = np.stack([((parity >> (39 - i)) & 1).astype(np.uint8) for i in range(40)], axis=-1)
    return np.packbits(bits, axis=-1)


def gsm_fire_numpy(frames, max_burst: int = 12, lsb_first: bool = False):
    """the rule of vit_hip_gsm_fire_batch on the host: frames uint8 [F][28] -> (status int32 [F][4] = (status, first_bit, syndrome_lo,
    syndrome_hi), the last three the uint32 values of the ABI; data uint8 [F][23]).  Error trapping: the syndrome is divided by D until it
    is a pattern with p(0) = 1 of degree below max_burst at a shift m with m + degree <= 223"""
    frames = np.asarray(frames, dtype=np.uint8)
    max_burst = int(max_burst)
    if frames.ndim != 2 or frames.shape[1] != 28 or not 0 <= max_burst <= 12:
        raise ValueError("frames must be uint8 [F][28], max_burst 0 .. 12")
    bits = np.unpackbits(frames, axis=1)
    syndromes = _fire_remainder(bits) ^ ((1 << 40) - 1)
    status = np.zeros((frames.shape[0], 4), dtype=np.uint32)
    for f, syndrome in enumerate(syndromes):
        syndrome = int(syndrome)
        status[f, 2], status[f, 3] = syndrome & 0xFFFFFFFF, syndrome >> 32
        if syndrome == 0:
            continue
        status[f, 0] = 0xFFFFFFFF
        p = syndrome
        for m in range(224 if max_burst else 0):
            if p & 1 and p >> max_burst == 0 and m + p.bit_length() - 1 <= 223:
                degree = p.bit_length() - 1
                status[f, 0], status[f, 1] = degree + 1, 223 - m - degree
                for i in range(degree + 1):
                    bits[f, 223 - m - i] ^= (p >> i) & 1
                break
            p = (p ^ GSM_FIRE_G if p & 1 else p) >> 1
    data = np.packbits(bits[:, :184], axis=1, bitorder="little" if lsb_first else "big")
    return status.view(np.int32), data


def gsm_tchfs_numpy(bytes, class2, high: int, low: int):
    """the rule of vit_hip_gsm_tchfs_batch on the host: bytes uint8 [F][24] (u(0 .. 184) MSB-first) and class2 [F][78] soft values ->
    (speech uint8 [F][33], status int32 [F][2] = (parity_syndrome, class2_erasures))"""
    bytes, class2 = np.asarray(bytes, dtype=np.uint8), np.asarray(class2)
    if bytes.ndim != 2 or bytes.shape[1] != 24 or class2.shape != (bytes.shape[0], 78):
        raise ValueError("bytes must be uint8 [F][24], class2 [F][78]")
    u = np.unpackbits(bytes, axis=1)[:, :185]
    d = np.zeros((bytes.shape[0], 264), dtype=np.uint8)
    d[:, 0:182:2], d[:, 1:182:2] = u[:, :91], u[:, 184:93:-1]
    twice = 2 * class2.astype(np.int64) - (int(high) + int(low))
    d[:, 182:260] = twice > 0
    framed = np.packbits(np.concatenate([d[:, :50], u[:, 91:94]], axis=1), axis=1)
    syndrome = crc_numpy(GSM_TCHFS_CRC3, framed, 50) ^ (u[:, 91] * 4 + u[:, 92] * 2 + u[:, 93])
    return np.packbits(d, axis=1), np.stack([syndrome, (twice == 0).sum(axis=1)], axis=1).astype(np.int32)


def _coded(frame_bytes, L, polynomials):
    """the 2 (L + 4) coded bits of every frame of uint8 [n][ceil(L / 8)], c[2 t + o] = polynomial o of step t"""
    return encode_bits_numpy(5, 2, polynomials, np.asarray(frame_bytes, dtype=np.uint8))[:, :L + 4].reshape(len(frame_bytes), -1)


def _soft(bits, amplitude, dtype):
    return np.where(np.asarray(bits) != 0, int(amplitude), -int(amplitude)).astype(dtype)


def gsm_xcch_bursts_numpy(l2, polynomials=GSM_POLYNOMIALS, amplitude: int = 127, dtype=np.int16):
    """the transmit side of a control channel, for tests: l2 uint8 [n][23] -> bursts [4 n][116] of +-amplitude as received without noise:
    Fire parity, 4 tail bits, the code, the block interleaver; both stealing flags of every burst 1, as SACCH sends them"""
    l2 = np.asarray(l2, dtype=np.uint8)
    coded = _coded(gsm_fire_encode_numpy(l2), 224, polynomials)
    burst, element = gsm_interleave_map(GSM_BLOCK)
    out = np.full((l2.shape[0], 4, GSM_BURST), int(amplitude), dtype=dtype)
    out[:, burst, element] = _soft(coded, amplitude, dtype)
    return out.reshape(-1, GSM_BURST)


def gsm_tchfs_class1_numpy(speech):
    """speech uint8 [n][33] (260 bits MSB-first) -> the 24 bytes of u(0 .. 184): the class I bits reordered around the 3 parity bits"""
    d = np.unpackbits(np.asarray(speech, dtype=np.uint8), axis=1)
    u = np.zeros((d.shape[0], 192), dtype=np.uint8)
    u[:, :91], u[:, 184:93:-1] = d[:, 0:182:2], d[:, 1:182:2]
    parity = crc_numpy(GSM_TCHFS_CRC3, np.packbits(d[:, :56], axis=1), 50)
    u[:, 91], u[:, 92], u[:, 93] = (parity >> 2) & 1, (parity >> 1) & 1, parity & 1
    return np.packbits(u, axis=1)


def gsm_tchfs_bursts_numpy(speech, polynomials=GSM_POLYNOMIALS, amplitude: int = 127, dtype=np.int16):
    """the transmit side of TCH/FS, for tests: speech uint8 [n][33] -> bursts [4 n + 4][116]: class I coded, class II uncoded behind it,
    the diagonal interleaver; stealing flags 0; the halves no block fills -- the odd positions of the first four bursts, the even ones of
    the last four -- are 0, the erasure"""
    speech = np.asarray(speech, dtype=np.uint8)
    n = speech.shape[0]
    coded = np.concatenate([_coded(gsm_tchfs_class1_numpy(speech), 185, polynomials), np.unpackbits(speech, axis=1)[:, 182:260]], axis=1)
    burst, element = gsm_interleave_map(GSM_DIAGONAL)
    out = np.zeros((4 * n + 4, GSM_BURST), dtype=dtype)
    out[:, 57:59] = -int(amplitude)
    for b in range(n):
        out[4 * b + burst, element] = _soft(coded[b], amplitude, dtype)
    return out


def gsm_facch_steal_numpy(bursts, block: int, l2, polynomials=GSM_POLYNOMIALS, amplitude: int = 127):
    """FACCH/F steals speech block `block` of a gsm_tchfs_bursts_numpy sequence, in place: the 456 coded bits of l2 uint8 [23] overwrite
    the even positions of bursts 4 block .. + 3 and the odd ones of the next four, and the flags of those halves (hu of the first four,
    hl of the last four) are set to 1.  returns bursts"""
    coded = _coded(gsm_fire_encode_numpy(np.asarray(l2, dtype=np.uint8).reshape(1, 23)), 224, polynomials)[0]
    burst, element = gsm_interleave_map(GSM_DIAGONAL)
    bursts[4 * block + burst, element] = _soft(coded, amplitude, bursts.dtype)
    bursts[4 * block:4 * block + 4, 58] = int(amplitude)
    bursts[4 * block + 4:4 * block + 8, 57] = int(amplitude)
    return bursts


class GsmControlDecoder:
    """a control channel (SACCH, BCCH, CCCH, SDCCH) on the card, from bursts to L2 frames: block de-interleave, decode with L = 224, the Fire
    code -- three calls, no host synchronisation, no memset, capturable as one graph once the buffers stand (they are allocated at the
    first push of a shape, the decision workspace too).  dec: a BatchDecoder of K = 5, R = 1/2, GSM_POLYNOMIALS for a real network"""

    def __init__(self, dec, max_burst: int = 12, negate: bool = False, lsb_first: bool = False):
        if (dec.K, dec.R) != (5, 2):
            raise ValueError("GsmControlDecoder needs a K = 5, R = 1/2 decoder")
        self.dec, self.max_burst, self.negate, self.lsb_first = dec, int(max_burst), bool(negate), bool(lsb_first)
        self._shape = None

    def push(self, bursts, out=None):
        """bursts: [rows][4 m][116] (or [4 m][116]: one row) of the decoder's symbol dtype on its device.  returns (l2 uint8 [rows * m][23],
        fire_status int32 [rows * m][4] = (status, first_bit, syndrome_lo, syndrome_hi)); out = the same two reuses those tensors"""
        from .is95 import _decode
        d, t = self.dec, self.dec.torch
        rows, m = (1 if bursts.dim() == 2 else int(bursts.shape[0])), int(bursts.shape[-2]) // 4
        if (rows, m) != self._shape:
            self._full = d._empty((rows, m, 228, 2), d._soft_dtype)
            self._bytes = d._empty((rows * m, 28), t.uint8)
            self._ws = d.new_workspace(rows * m, 224)
            self._shape = (rows, m)
        if out is None:
            out = (d._empty((rows * m, 23), t.uint8), d._empty((rows * m, 4), t.int32))
        d.gsm_deinterleave(bursts, GSM_BLOCK, negate=self.negate, out={"full": self._full})
        _decode(d, self._full.view(rows * m, 228, 2), 224, self._ws, self._bytes)
        status, l2 = d.gsm_fire(self._bytes, self.max_burst, lsb_first=self.lsb_first, out=(out[1], out[0]))
        return l2, status


class GsmTchfDecoder:
    """a full-rate traffic channel on the card, from bursts to speech frames and FACCH frames: the diagonal de-interleave with its four
    bursts of history, then every block BOTH ways, as the IS-95 receiver decodes all rates -- decode with L = 185 and the TCH/FS frame,
    decode with L = 224 and the Fire code -- five calls, no host synchronisation, no memset.  The caller picks by `steal` (above the
    midpoint: FACCH) and the two checks.  The history travels between two buffers of the receiver's from push to push, so a graph
    captures an EVEN number of pushes.  dec: a BatchDecoder of K = 5, R = 1/2"""

    def __init__(self, dec, max_burst: int = 12, negate: bool = False, lsb_first: bool = False):
        if (dec.K, dec.R) != (5, 2):
            raise ValueError("GsmTchfDecoder needs a K = 5, R = 1/2 decoder")
        self.dec, self.max_burst, self.negate, self.lsb_first = dec, int(max_burst), bool(negate), bool(lsb_first)
        self._shape, self._state, self._turn, self.n_out = None, None, 0, None

    def reset(self):
        """forget the history: the next push starts a new sequence of bursts"""
        if self._state is not None:
            for _, fill in self._state:
                fill.zero_()

    def push(self, bursts, out=None):
        """bursts: [rows][4 m][116] (or [4 m][116]: one row), the next 4 m bursts of every row.  returns (speech uint8 [n][33], parity int32
        [n][2] = (parity_syndrome, class2_erasures), facch uint8 [n][23], fire_status int32 [n][4], steal int32 [n]) with n = rows * m
        slots, row r's blocks in slots r * m ..; the first push of a sequence fills m - 1 of a row's slots and leaves the last as the
        de-interleaver's zeros decode, and self.n_out (int32 [rows], on the device) says how many.  out = the same five reuses those
        tensors"""
        from .is95 import _decode
        d, t = self.dec, self.dec.torch
        rows, m = (1 if bursts.dim() == 2 else int(bursts.shape[0])), int(bursts.shape[-2]) // 4
        n = rows * m
        if (rows, m) != self._shape:
            self._full, self._class1 = d._empty((rows, m, 228, 2), d._soft_dtype), d._empty((rows, m, 189, 2), d._soft_dtype)
            self._class2 = d._empty((rows, m, 78), d._soft_dtype)
            self._b224, self._b185 = d._empty((n, 28), t.uint8), d._empty((n, 24), t.uint8)
            self._ws = (d.new_workspace(n, 224), d.new_workspace(n, 185))
            self.n_out = d._empty((rows,), t.int32)
            if self._state is None or self._state[0][0].shape[0] != rows:
                self._state = tuple((d._empty((rows, 4 * GSM_BURST), d._soft_dtype), t.zeros(rows, dtype=t.int32, device=d.device)) for _ in range(2))
                self._turn = 0
            self._shape = (rows, m)
        if out is None:
            out = (d._empty((n, 33), t.uint8), d._empty((n, 2), t.int32), d._empty((n, 23), t.uint8), d._empty((n, 4), t.int32),
                   d._empty((n,), t.int32))
        speech, parity, facch, fire, steal = out
        (hist, fill), (hist_out, fill_out) = self._state[self._turn], self._state[1 - self._turn]
        self._turn = 1 - self._turn
        d.gsm_deinterleave(bursts, GSM_DIAGONAL, negate=self.negate, hist=hist, fill=fill,
                           out={"full": self._full, "class1": self._class1, "class2": self._class2, "steal": steal.view(rows, m),
                                "n_out": self.n_out, "hist_out": hist_out, "fill_out": fill_out})
        _decode(d, self._class1.view(n, 189, 2), 185, self._ws[1], self._b185)
        d.gsm_tchfs(self._b185, self._class2.view(n, 78), out=(speech, parity))
        _decode(d, self._full.view(n, 228, 2), 224, self._ws[0], self._b224)
        d.gsm_fire(self._b224, self.max_burst, lsb_first=self.lsb_first, out=(fire, facch))
        return speech, parity, facch, fire, steal
