"""What the IS-95A traffic channel tests share: a set of forward traffic frames of mixed rates as Walsh-despread soft symbols, noise-free or
in white Gaussian noise, and the CPU composition of the receive chain -- the numpy rules of viterbidecodercpp_amd/is95.py around the oracle
decoder -- that the GPU chain is compared with."""
import functools

import numpy as np

from oracle import pyoracle
from viterbidecodercpp_amd import (COMMON_CODES, IS95_POLYNOMIALS, IS95_RATE_SET_1, crc_field_numpy, crc_numpy, is95_deinterleave_numpy,
                                   is95_rate_decide_numpy, is95_traffic_frame_numpy)
from viterbidecodercpp_amd.codes import Code
from viterbidecodercpp_amd.synth import channel_errors_numpy, encode_bits_numpy

STOCK = COMMON_CODES[5]
assert STOCK.name == "CDMA IS-95A"
CODES = {"stock": STOCK, "standard": Code("IS-95A as the standard reads", 9, 2, IS95_POLYNOMIALS)}

# The noisy set.  Chosen on the CPU: at this seed and Es/N0 per received symbol the chain by the host rules below returns the sent rate, the
# sent info bits and (h < 2) a zero syndrome for EVERY one of the 64 frames at both polynomial sets, with MAX_SER as the threshold -- a
# condition on the inputs, not a tolerance on the GPU.  AMPLITUDE 40 of 127: the raw symbol error rate is about 4 %, so the full-rate
# decodes correct some fifteen symbols a frame, and sums of eight saturate at the clamp as they would in a receiver.
NOISY_FRAMES, NOISY_SEED, NOISY_SNR_DB, AMPLITUDE = 64, 95, 2.0, 40
MAX_SER = ((1, 1, 1, 1), 10)                                       # errors / compared <= 1 / 10 at every hypothesis
HIGH, LOW = 127, -127


def make_frames(code, frames=NOISY_FRAMES, seed=NOISY_SEED, snr_db=None):
    """-> (symbols int16 [frames][384], scramble uint8 [frames][48], rates [frames], info uint8 [frames][22]: the sent info bits, zero
    behind them).  Rates go round 0, 1, 2, 3 with a random start per group of four; every frame has a long-code mask of its own.
    Noise-free the symbols are +-127; with snr_db they are AMPLITUDE (+-1 + n), n white Gaussian of variance 1 / (2 snr), rounded and
    clipped to [-127, 127]"""
    rng = np.random.default_rng(seed)
    rates = np.concatenate([rng.permutation(4) for _ in range(-(-frames // 4))])[:frames]
    scramble = rng.integers(0, 256, size=(frames, 48), dtype=np.uint8)
    symbols = np.empty((frames, 384), dtype=np.int16)
    info = np.zeros((frames, 22), dtype=np.uint8)
    for f, h in enumerate(rates):
        bits = rng.integers(0, 2, size=IS95_RATE_SET_1[h].info_bits, dtype=np.uint8)
        symbols[f], _ = is95_traffic_frame_numpy(bits, h, scramble[f], polynomials=code.G)
        info[f] = np.packbits(np.concatenate([bits, np.zeros(176 - bits.size, dtype=np.uint8)]))
    if snr_db is not None:
        sigma = np.sqrt(0.5 / 10.0 ** (snr_db / 10.0))
        noisy = np.sign(symbols) + sigma * rng.standard_normal(symbols.shape)
        symbols = np.clip(np.rint(AMPLITUDE * noisy), LOW, HIGH).astype(np.int16)
    return symbols, scramble, rates, info


@functools.lru_cache(maxsize=None)
def _oracle():
    pyoracle.ensure_built()
    return pyoracle.Oracle()


def cpu_stages(code, symbols, scramble, shift=0):
    """the de-interleave, the four decodes, the four error counts and the two frame checks on the CPU -> (symbols per hypothesis, decoded
    bytes per hypothesis, errors, compared, syndromes [2][F])"""
    sym = is95_deinterleave_numpy(symbols, scramble, shift, LOW, HIGH)
    decoded, errors, compared, syndrome = [], [], [], []
    for h, r in enumerate(IS95_RATE_SET_1):
        b = _oracle().decode_frames(9, 2, code.G, pyoracle.stock_config(pyoracle.SOFT16, 2), sym[h], r.L)[0]
        e, c = channel_errors_numpy(code, HIGH, LOW, sym[h], encode_bits_numpy(9, 2, code.G, b))
        decoded.append(b), errors.append(e), compared.append(c)
        if r.crc is not None:
            syndrome.append(crc_numpy(r.crc, b, r.info_bits) ^ crc_field_numpy(r.crc, b, r.info_bits))
    return sym, decoded, errors, compared, syndrome


def cpu_chain(code, symbols, scramble, max_ser=MAX_SER, shift=0):
    """the twelve stages on the CPU -> (decision uint32 [F][4], info uint8 [F][22], syndromes [2][F], (errors, compared) per hypothesis)"""
    _, decoded, errors, compared, syndrome = cpu_stages(code, symbols, scramble, shift)
    decision, info = is95_rate_decide_numpy(decoded, errors, compared, syndrome, max_ser[0], max_ser[1])
    return decision, info, syndrome, list(zip(errors, compared))


@functools.lru_cache(maxsize=None)
def noisy_set(name):
    """the noisy set of one polynomial set ("stock" or "standard") and what the CPU chain makes of it, computed once"""
    code = CODES[name]
    symbols, scramble, rates, info = make_frames(code, snr_db=NOISY_SNR_DB)
    return symbols, scramble, rates, info, cpu_chain(code, symbols, scramble)
