"""An independent restatement of the 802.11a/g OFDM data path, in plain Python lists and loops, for the tests of viterbidecodercpp_amd/wifi.py
and of the vit_hip_wifi_* calls: the interleaver as the standard's two permutations applied on the transmit side and inverted by table,
puncturing as a mask walked bit by bit, the scrambler as a 7-bit shift register stepped bit by bit, the FCS by zlib.crc32."""
import zlib

# Mbit/s, N_BPSC, puncturing mask over A1 B1 A2 B2 ..., N_CBPS, N_DBPS, R1 R2 R3 R4
RATES = [
    (6, 1, [1, 1], 48, 24, [1, 1, 0, 1]), (9, 1, [1, 1, 1, 0, 0, 1], 48, 36, [1, 1, 1, 1]),
    (12, 2, [1, 1], 96, 48, [0, 1, 0, 1]), (18, 2, [1, 1, 1, 0, 0, 1], 96, 72, [0, 1, 1, 1]),
    (24, 4, [1, 1], 192, 96, [1, 0, 0, 1]), (36, 4, [1, 1, 1, 0, 0, 1], 192, 144, [1, 0, 1, 1]),
    (48, 6, [1, 1, 1, 0], 288, 192, [0, 0, 0, 1]), (54, 6, [1, 1, 1, 0, 0, 1], 288, 216, [0, 0, 1, 1]),
]
POISON16, POISON8 = 0x5A5A, 0x5A


def first_permutation(n_cbps):
    """k -> i: adjacent coded bits go to non-adjacent subcarriers"""
    return [(n_cbps // 16) * (k % 16) + k // 16 for k in range(n_cbps)]


def second_permutation(n_cbps, n_bpsc):
    """i -> j: adjacent coded bits alternate between more and less significant bits of the constellation"""
    s = max(n_bpsc // 2, 1)
    return [s * (i // s) + (i + n_cbps - 16 * i // n_cbps) % s for i in range(n_cbps)]


def interleave_symbol(coded, n_bpsc):
    """one OFDM symbol on the transmit side: first permutation, then the second"""
    n = len(coded)
    after_first = [None] * n
    for k, i in enumerate(first_permutation(n)):
        after_first[i] = coded[k]
    sent = [None] * n
    for i, j in enumerate(second_permutation(n, n_bpsc)):
        sent[j] = after_first[i]
    return sent


def interleave_table(rate):
    """table[k] = the transmitted place of coded bit k, found by sending the numbers 0 .. N_CBPS - 1 through the transmit side"""
    _, n_bpsc, _, n_cbps, _, _ = RATES[rate]
    sent = interleave_symbol(list(range(n_cbps)), n_bpsc)
    table = [None] * n_cbps
    for j, k in enumerate(sent):
        table[k] = j
    return table


def deinterleave(frame, rate, max_sym, S, n_sym=None, n_steps=None):
    """one frame (a list of soft bits) -> the 2 S values of [S][2]; rate above 7: all erased"""
    out = [0] * (2 * S)
    if not 0 <= rate <= 7:
        return out
    _, _, mask, n_cbps, n_dbps, _ = RATES[rate]
    n_sym = min(max_sym if n_sym is None else n_sym, max_sym)
    limit = n_sym * n_dbps
    n_steps = min(limit if n_steps is None else n_steps, limit, S)
    table = interleave_table(rate)
    c = 0
    for q in range(2 * n_steps):
        if mask[q % len(mask)]:
            y, k = divmod(c, n_cbps)
            out[q] = frame[y * n_cbps + table[k]]
            c += 1
    return out


def bits_of(data, n):
    """the first n bits of bytes, bit t being bit 7 - t%8 of byte t/8"""
    return [(data[t // 8] >> (7 - t % 8)) & 1 for t in range(n)]


def signal_parse(three_bytes):
    """(rate_index, length, n_sym, n_steps, valid) of the SIGNAL field's decoded bytes"""
    b = bits_of(three_bytes, 18)
    rate = 8
    for m, row in enumerate(RATES):
        if row[5] == b[:4]:
            rate = m
    length = sum(b[5 + i] << i for i in range(12))
    valid = rate < 8 and sum(b[:18]) % 2 == 0 and b[4] == 0 and length >= 1
    if not valid:
        return (rate, length, 0, 0, 0)
    n_steps = 16 + 8 * length + 6
    return (rate, length, (n_steps + RATES[rate][4] - 1) // RATES[rate][4], n_steps, 1)


def shift_register(state, n):
    """n output bits of the scrambler x^7 + x^4 + 1 from `state` = [x1 .. x7]"""
    x = list(state)
    out = []
    for _ in range(n):
        bit = x[3] ^ x[6]
        out.append(bit)
        x = [bit] + x[:6]
    return out


def sequence_from(first_seven, n):
    """the scrambling sequence whose first seven bits are given: the register state that produces them, by trying all 128"""
    for v in range(128):
        state = [(v >> i) & 1 for i in range(7)]
        if shift_register(state, 7) == list(first_seven):
            return shift_register(state, n)
    raise AssertionError("no state gives these seven bits")


def descramble(data, S, length, max_length=4095):
    """(psdu octets, (length_used, seed, service, fcs_syndrome)) of one DATA field's decoded bytes"""
    n_bits = S - 6
    d = bits_of(data, n_bits)
    u = [a ^ b for a, b in zip(d, sequence_from(d[:7], n_bits))]
    n = min(length, max_length, (n_bits - 16) // 8)
    psdu = bytes(sum(u[16 + 8 * g + b] << b for b in range(8)) for g in range(n))
    syndrome = zlib.crc32(psdu[:-4]) ^ int.from_bytes(psdu[-4:], "little") if n >= 4 else 0xFFFFFFFF
    return psdu, (n, sum(d[i] << (6 - i) for i in range(7)), sum(u[i] << i for i in range(16)), syndrome)
