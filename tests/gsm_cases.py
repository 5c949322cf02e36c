"""What the GSM tests share: Fire-code frames with every kind of damage, control-channel and TCH/F burst sequences with a fixed set of
sign flips, and the CPU composition of the two receive chains -- the numpy rules of viterbidecodercpp_amd/gsm.py around the oracle
decoder -- that the GPU chains are compared with.  Everything is computed once and shared."""
import functools

import numpy as np

from oracle import pyoracle
from viterbidecodercpp_amd import (GSM_BLOCK, GSM_DIAGONAL, GSM_POLYNOMIALS, gsm_deinterleave_numpy, gsm_facch_steal_numpy, gsm_fire_encode_numpy,
                                   gsm_fire_numpy, gsm_interleave_map, gsm_tchfs_bursts_numpy, gsm_tchfs_numpy, gsm_xcch_bursts_numpy)
from viterbidecodercpp_amd.codes import Code

CODE = Code("GSM K=5 R=1/2", 5, 2, GSM_POLYNOMIALS)
HIGH, LOW = 127, -127
# The sign flips.  Chosen on the CPU: with FLIPS coded bits of every block negated at places drawn from this seed -- class I and control
# bits only: class II is uncoded -- the chains by the host rules below return every sent frame: a condition on the inputs, not a
# tolerance on the GPU
SEED, FLIPS = 45, 5
STOLEN = 3                                                          # the speech block FACCH steals


@functools.lru_cache(maxsize=None)
def _oracle():
    pyoracle.ensure_built()
    return pyoracle.Oracle()


def decode(symbols, L):
    """the oracle's decode of [F][L + 4][2] int16 -> uint8 [F][ceil(L / 8)]"""
    return _oracle().decode_frames(5, 2, CODE.G, pyoracle.stock_config(pyoracle.SOFT16, 2), np.ascontiguousarray(symbols), L)[0]


@functools.lru_cache(maxsize=None)
def fire_frames():
    """uint8 [256][28]: clean frames; every kind of burst of length 1 .. 12 at first bits 0, 100, 212 (or the last place the burst fits)
    and 223 - length + 1, data and parity alike; single-bit errors; 13-bit bursts; two errors far apart.  -> (frames, what was sent)"""
    rng = np.random.default_rng(40)
    sent = gsm_fire_encode_numpy(rng.integers(0, 256, size=(256, 23), dtype=np.uint8))
    bits = np.unpackbits(sent, axis=1)
    f = 8                                                           # frames 0 .. 7 stay clean
    for length in range(1, 13):
        for t0 in sorted({0, 100, min(212, 224 - length), 224 - length}):
            bits[f, t0] ^= 1
            bits[f, t0 + length - 1] ^= length > 1
            if length > 2:
                bits[f, t0 + 1:t0 + length - 1] ^= rng.integers(0, 2, size=length - 2, dtype=np.uint8)
            f += 1
    for t in (0, 1, 7, 8, 63, 64, 127, 128, 183, 184, 185, 191, 192, 222, 223):
        bits[f, t] ^= 1
        f += 1
    for t0 in (0, 50, 150, 211):                                    # thirteen bits: both ends flipped
        bits[f, t0] ^= 1
        bits[f, t0 + 12] ^= 1
        f += 1
    for a, b in ((0, 223), (3, 100), (90, 130), (183, 184 + 20)):   # two errors, separated
        bits[f, a] ^= 1
        bits[f, b] ^= 1
        f += 1
    while f < 256:                                                  # the rest: a random burst each, or noise
        length = int(rng.integers(1, 13))
        t0 = int(rng.integers(0, 224 - length + 1))
        if f % 8 == 7:
            bits[f] ^= rng.integers(0, 2, size=224, dtype=np.uint8)
        else:
            bits[f, t0] ^= 1
            bits[f, t0 + length - 1] ^= length > 1
        f += 1
    return np.packbits(bits, axis=1), sent


def flip(bursts, blocks, mode, rng, limit):
    """negate FLIPS coded bits below `limit` of every block of a burst sequence [..][116], in place"""
    burst, element = gsm_interleave_map(mode)
    for n in range(blocks):
        k = rng.choice(limit, size=FLIPS, replace=False)
        bursts[4 * n + burst[k], element[k]] *= -1
    return bursts


@functools.lru_cache(maxsize=None)
def control_set():
    """8 random L2 frames on a control channel -> (bursts int16 [1][32][116], l2 uint8 [8][23], (l2, fire status) of the host chain)"""
    rng = np.random.default_rng(SEED)
    l2 = rng.integers(0, 256, size=(8, 23), dtype=np.uint8)
    bursts = flip(gsm_xcch_bursts_numpy(l2), 8, GSM_BLOCK, rng, 456)[None]
    return bursts, l2, control_chain(bursts)


def control_chain(bursts, max_burst=12, lsb_first=False):
    full = gsm_deinterleave_numpy(bursts, GSM_BLOCK)[0]
    status, data = gsm_fire_numpy(decode(full.reshape(-1, 228, 2), 224), max_burst, lsb_first)
    return data, status


@functools.lru_cache(maxsize=None)
def traffic_set():
    """8 speech frames, block STOLEN replaced by a FACCH frame -> (bursts int16 [36][116], speech uint8 [8][33], l2 uint8 [23])"""
    rng = np.random.default_rng(SEED + 1)
    speech = np.packbits(np.concatenate([rng.integers(0, 2, size=(8, 260), dtype=np.uint8), np.zeros((8, 4), dtype=np.uint8)], axis=1), axis=1)
    l2 = rng.integers(0, 256, size=23, dtype=np.uint8)
    bursts = gsm_facch_steal_numpy(gsm_tchfs_bursts_numpy(speech), STOLEN, l2)
    bursts = flip(bursts, 8, GSM_DIAGONAL, rng, 378)
    return bursts, speech, l2


def traffic_chain(pushes, max_burst=12):
    """the TCH/F receiver on the host: pushes, a list of arrays [rows][4 m][116], the history carried from one to the next -> per push
    (speech, parity, facch, fire, steal, n_out), every array over rows * m slots"""
    hist = fill = None
    out = []
    for bursts in pushes:
        full, class1, class2, steal, n_out, hist, fill = gsm_deinterleave_numpy(bursts, GSM_DIAGONAL, hist=hist, fill=fill)
        speech, parity = gsm_tchfs_numpy(decode(class1.reshape(-1, 189, 2), 185), class2.reshape(-1, 78), HIGH, LOW)
        fire, facch = gsm_fire_numpy(decode(full.reshape(-1, 228, 2), 224), max_burst)
        out.append((speech, parity, facch, fire, steal.reshape(-1), n_out))
    return out
