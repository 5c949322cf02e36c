"""What the DVB-T tests share: the transmit side from transport packets to the demapper's soft bits, noise-free or in white Gaussian
noise; the chain by the host rules alone -- the numpy rules of viterbidecodercpp_amd/dvbt.py and dvb.py around a maximum-likelihood
decode in numpy -- that the GPU chain is compared with; and the pushes through a DvbtDecoder.  tests/test_gpu_dvbt.py and
tests/test_gpu_dvbt_edges.py run them on the card, tests/test_dvbt_cpu.py holds transmit() to the values it had when the first was
written."""
import numpy as np

from viterbidecodercpp_amd import (COMMON_CODES, DVB_INTERLEAVER, DVB_RS_204_188, DvbtDecoder, conv_deinterleave_numpy, conv_interleave_numpy,
                                   dvb_derandomize_numpy, dvb_randomize_numpy, dvbt_deinterleave_numpy, dvbt_interleave_numpy, dvbt_puncture_numpy,
                                   dvbt_steps_per_symbol, get_decoding_config, rs_decode_numpy, rs_encode_numpy)
from viterbidecodercpp_amd.synth import encode_bits_numpy

AMPLITUDE = 48          # of a soft bit under noise: 127 is 2.8 sigma away at the lowest SNR used, so few values clip and magnitudes are real
# Es/N0 of one sent soft bit in dB, by rate index: where EN 300 421 table 5 puts quasi-error-free reception of this inner code behind
# RS(204,188) -- Eb/N0 of 4.5, 5.0, 5.5, 6.0 and 6.4 dB at 1/2, 2/3, 3/4, 5/6 and 7/8, less 10 log10 of the rate's reciprocal.  The channel
# bit error rate is 4.4 %, 1.0 % and 0.26 % at 1/2, 3/4 and 7/8, and what the decode leaves is Reed-Solomon's to correct.  The host-rule
# chain recovers every packet there
SNR_DB = {0: 1.5, 1: 3.25, 2: 4.25, 3: 5.2, 4: 5.8}
NOISE_SEED = 2024
FORNEY_DELAY = 11       # packets that fill the delay lines of the (12, 17) de-interleaver behind a lock and give no output


def transmit(mode, v, rate, n_packets, seed, pc, snr_db=None, noise_seed=None, parity=0, decode_type=None):
    """random transport packets -> energy dispersal, RS(204,188), Forney (12, 17), the package's encoder rule, puncturing, the inner
    interleaver -> soft bits [n_sym][Nmax * v] from symbol parity `parity`, the last symbol padded with random bits.  The symbol type and
    its levels are those of pc, or with decode_type ("SOFT16", "SOFT8", "HARD8") of that type's stock configuration (pc may be None).
    Noise-free they are high / low; with snr_db every soft bit is amplitude (+-1 + n), amplitude = AMPLITUDE of a high of 127, n white
    Gaussian of variance 1 / (2 snr) -- snr = Es/N0 of one sent bit -- from noise_seed, rounded and clipped to [low, high]"""
    if decode_type is not None:
        pc = get_decoding_config(decode_type, 2)
    rng = np.random.default_rng(seed)
    ts = rng.integers(0, 256, size=(n_packets, 188), dtype=np.uint8)
    ts[:, 0] = 0x47
    sent = conv_interleave_numpy(rs_encode_numpy(DVB_RS_204_188, dvb_randomize_numpy(ts), 1), *DVB_INTERLEAVER)
    steps = dvbt_steps_per_symbol(mode, v, rate)
    bits = np.unpackbits(sent.reshape(-1))
    n_sym = -(-(bits.size + 6) // steps)
    bits = np.concatenate([bits, rng.integers(0, 2, size=n_sym * steps - bits.size, dtype=np.uint8)])
    coded = encode_bits_numpy(7, 2, COMMON_CODES[2].G, np.packbits(bits))[0, :bits.size]
    cells = dvbt_interleave_numpy(dvbt_puncture_numpy(coded, rate), mode, v, parity)
    if snr_db is None:
        return ts, np.where(cells != 0, pc.soft_decision_high, pc.soft_decision_low).astype(pc.soft_dtype)
    amplitude = AMPLITUDE * int(pc.soft_decision_high) // 127
    sigma = np.sqrt(0.5 / 10.0 ** (snr_db / 10.0))
    noisy = np.where(cells != 0, 1.0, -1.0) + sigma * np.random.default_rng(noise_seed).standard_normal(cells.shape)
    return ts, np.clip(np.rint(amplitude * noisy), pc.soft_decision_low, pc.soft_decision_high).astype(pc.soft_dtype)


def viterbi_numpy(steps):
    """the host rule of the decode: the maximum-likelihood path of the stock K = 7 code from the zero state through steps [n][2] (0 an
    erasure), by correlation in int64, chained back from the best final state -> bits uint8 [n]"""
    new = np.arange(64)
    reg = new[:, None] | (np.arange(2)[None, :] << 6)               # [new state][oldest bit]: bit k is the input of k steps ago
    prev = reg >> 1
    sign = np.stack([2 * (sum((reg & g) >> k & 1 for k in range(7)) & 1) - 1 for g in COMMON_CODES[2].G], axis=-1).astype(np.int64)
    y = np.asarray(steps).astype(np.int64)
    branch = sign[None, :, :, 0] * y[:, None, None, 0] + sign[None, :, :, 1] * y[:, None, None, 1]
    metric = np.full(64, -1 << 40, dtype=np.int64)
    metric[0] = 0
    chose = np.empty((len(y), 64), dtype=np.uint8)
    for t in range(len(y)):
        cand = metric[prev] + branch[t]
        chose[t] = cand[:, 1] > cand[:, 0]
        metric = cand.max(axis=1)
    state, bits, prev, chose = int(metric.argmax()), np.empty(len(y), dtype=np.uint8), prev.tolist(), chose.tolist()
    for t in range(len(y) - 1, -1, -1):
        bits[t] = state & 1
        state = prev[state][chose[t][state]]
    return bits


def host_chain(soft, mode, v, rate, n_packets, parity=0):
    """the receive chain by the host rules alone: dvbt_deinterleave_numpy, the decode, the Forney de-interleaver, RS(204,188), energy
    dispersal.  The stream starts at a packet, so the host needs no sync search -> (packets [n_packets - 11][188], rs_status)"""
    bits = viterbi_numpy(dvbt_deinterleave_numpy(soft, mode, v, rate, parity))
    frames = np.packbits(bits[:n_packets * 1632]).reshape(n_packets, 204)
    frames, status = rs_decode_numpy(DVB_RS_204_188, conv_deinterleave_numpy(frames, *DVB_INTERLEAVER)[0])
    return dvb_derandomize_numpy(frames, 0)[0], status.reshape(-1)


def receive_all(dec, mode, v, rate, soft, cuts, window=1024, **kw):
    """soft [n_sym][Nmax * v], or with n_streams=n in kw [n][n_sym][Nmax * v], through one DvbtDecoder(dec, mode, v, rate, window=window,
    **kw) in pushes cut at the symbol counts `cuts`, the last of them a finish(), with a take_frames() behind every one -> (packets,
    sync_errors, rs_status [k]) of all of them: the one triple, or with n_streams a list of one per stream"""
    import torch
    d = torch.from_numpy(soft).cuda()
    many = kw.get("n_streams") is not None
    n_sym = soft.shape[1] if many else len(soft)
    rx = DvbtDecoder(dec, mode, v, rate, window=window, **kw)
    taken = []
    edges = [0] + [c for c in cuts if c < n_sym] + [n_sym]
    for a, b in zip(edges[:-1], edges[1:]):
        part = d[:, a:b] if many else d[a:b]
        rx.finish(part) if b == n_sym else rx.push(part)
        got = rx.take_frames()
        taken.append(got if many else [got])
    streams = [tuple(np.concatenate([t[s][i] for t in taken]) for i in range(3)) for s in range(len(taken[0]))]
    streams = [(p, e, st.reshape(-1)) for p, e, st in streams]
    return streams if many else streams[0]


def receive(dec, mode, v, rate, soft, cuts):
    """soft [n_sym][Nmax * v] through a DvbtDecoder in pushes cut at `cuts` -> (packets, rs_status) of all its take_frames()"""
    packets, _, status = receive_all(dec, mode, v, rate, soft, cuts)
    return packets, status
