"""What the 802.11a/g tests share: PPDUs with a valid FCS as the demapper's soft bits -- int16 of +-127 for a SOFT16 decoder, int8 of +-3
for a SOFT8 one, the oracle's stock ranges --, SIGNAL fields of any 18 bits, and the CPU composition of the receive chain -- the numpy rules
of viterbidecodercpp_amd/wifi.py around the oracle decoder -- that the GPU chain is compared with."""
import zlib

import numpy as np

from oracle import pyoracle
from viterbidecodercpp_amd import (WIFI_POLYNOMIALS, WIFI_RATES, wifi_deinterleave_numpy, wifi_descramble_numpy, wifi_interleave_map,
                                   wifi_ppdu_numpy, wifi_signal_field_numpy, wifi_signal_parse_numpy)
from viterbidecodercpp_amd.synth import encode_bits_numpy

FILL = 0x5A
# decode type -> (the oracle's id, the soft bits' dtype, their amplitude: the stock configuration's soft_decision_high)
DECODE_TYPES = {"SOFT16": (pyoracle.SOFT16, np.int16, 127), "SOFT8": (pyoracle.SOFT8, np.int8, 3)}


def with_fcs(body: bytes) -> np.ndarray:
    """body + its FCS: a PSDU that checks"""
    return np.frombuffer(body + zlib.crc32(body).to_bytes(4, "little"), dtype=np.uint8)


def largest_length(rate: int, n_sym: int) -> int:
    """the longest PSDU whose DATA field fits n_sym OFDM symbols"""
    return (n_sym * WIFI_RATES[rate].n_dbps - 22) // 8


def signal_field_of_bits(bits18, amplitude=127, dtype=np.int16):
    """the SIGNAL symbol of ANY 18 bits (R1 R2 R3 R4, reserved, LENGTH LSB first, parity), conforming or not: six tail bits, rate 1/2,
    interleaved as one BPSK symbol -> 48 soft bits of +-amplitude.  wifi_signal_field_numpy for the fields a sender may not send"""
    bits = np.concatenate([np.asarray(bits18, dtype=np.uint8), np.zeros(6, dtype=np.uint8)])
    assert bits.size == 24
    coded = encode_bits_numpy(7, 2, WIFI_POLYNOMIALS, np.packbits(bits))[0, :24].reshape(-1)
    sent = np.empty_like(coded)
    sent[wifi_interleave_map(0)] = coded
    return np.where(sent != 0, amplitude, -amplitude).astype(dtype)


def signal_bits(rate: int, length: int):
    """the 18 bits a conforming sender puts into SIGNAL"""
    bits = np.zeros(18, dtype=np.uint8)
    bits[:4] = WIFI_RATES[rate].signal_bits
    bits[5:17] = (int(length) >> np.arange(12)) & 1
    bits[17] = bits[:17].sum() % 2
    return bits


def make_ppdus(specs, max_sym, seed=1, sigma=0.0, decode_type="SOFT16", signal_bits18=None):
    """specs: (rate, length, scrambler seed) per frame; a PSDU of four octets or more ends in its FCS -> (signal_soft [F][48], data_soft
    [F][max_sym * 288], psdus), soft bits of decode_type's dtype and amplitude.  Behind a frame's own symbols the row holds noise; sigma
    is the noise's standard deviation as a part of the amplitude, one for all frames or one per frame.  signal_bits18: {frame: 18 bits}
    that replace the frame's SIGNAL field"""
    _, dtype, amp = DECODE_TYPES[decode_type]
    rng = np.random.default_rng(seed)
    F = len(specs)
    signal_soft = np.zeros((F, 48), dtype=dtype)
    data_soft = rng.integers(-amp, amp + 1, size=(F, max_sym * 288)).astype(dtype)
    psdus = []
    for f, (rate, length, scr) in enumerate(specs):
        body = rng.integers(0, 256, size=max(length - 4, 0) if length >= 4 else length, dtype=np.uint8)
        psdu = with_fcs(body.tobytes()) if length >= 4 else body
        signal_soft[f] = wifi_signal_field_numpy(rate, length, amp, dtype)
        tx = wifi_ppdu_numpy(psdu, rate, scr, amp, dtype)
        assert tx.size <= max_sym * 288
        data_soft[f, :tx.size] = tx
        psdus.append(psdu)
    for f, bits in (signal_bits18 or {}).items():
        signal_soft[f] = signal_field_of_bits(bits, amp, dtype)
    if np.any(sigma):
        scale = np.asarray(sigma, dtype=np.float64) * amp
        scale = float(scale) if scale.ndim == 0 else scale.reshape(F, 1)
        noisy = lambda x: np.clip(np.rint(x + rng.normal(0.0, scale, size=x.shape)), -amp, amp).astype(dtype)
        signal_soft, data_soft = noisy(signal_soft), noisy(data_soft)
    return signal_soft, data_soft, psdus


_oracle = None


def oracle_decode(symbols, L, decode_type="SOFT16"):
    """[F][L + 6][2] soft bits -> bytes [F][ceil(L / 8)], by the CPU oracle decoder at decode_type's stock configuration"""
    global _oracle
    if _oracle is None:
        pyoracle.ensure_built()
        _oracle = pyoracle.Oracle()
    return _oracle.decode_frames(7, 2, WIFI_POLYNOMIALS, pyoracle.stock_config(DECODE_TYPES[decode_type][0], 2), symbols, L)[0]


def cpu_chain(signal_soft, data_soft, max_sym, decode_type="SOFT16"):
    """the six stages on the CPU -> (psdu image uint8 [F][max_length] over FILL, status uint32 [F][4], signal uint32 [F][5])"""
    S = max_sym * 216
    max_length = min((S - 22) // 8, 4095)
    signal = wifi_signal_parse_numpy(oracle_decode(wifi_deinterleave_numpy(signal_soft, 1, 24, rate=0), 18, decode_type))
    sym = wifi_deinterleave_numpy(data_soft, max_sym, S, rate=signal[:, 0], n_sym=signal[:, 2], n_steps=signal[:, 3])
    octets, status = wifi_descramble_numpy(oracle_decode(sym, S - 6, decode_type), S, signal[:, 1], max_length)
    image = np.full((len(octets), max_length), FILL, dtype=np.uint8)
    for f, o in enumerate(octets):
        image[f, :o.size] = o
    return image, status, signal
