"""An independent restatement of the GSM rules of include/vit_hip.h, in plain Python on lists, bit by bit: the interleaver as the
standard's forward scatter, the Fire syndrome by long division, the correction BY DEFINITION (every pattern of every length at every
position, kept where its flip zeroes the syndrome), the TCH/FS frame by the standard's sentences.  Shares no code with
viterbidecodercpp_amd/gsm.py."""

G = (1 << 40) | (1 << 26) | (1 << 23) | (1 << 17) | (1 << 3) | 1


def scatter(blocks, diagonal):
    """the transmit side: blocks, a list of lists of 456 values -> bursts, a list of lists of 116 (None where nothing was put): value k
    of block n goes to burst 4 n + (k mod 8 or k mod 4), position 2 ((49 k) mod 57) + ((k mod 8) div 4) of the 114, the flags between the
    halves"""
    bursts = [[None] * 116 for _ in range(4 * len(blocks) + (4 if diagonal else 0))]
    for n, block in enumerate(blocks):
        for k in range(456):
            j = 2 * ((49 * k) % 57) + ((k % 8) // 4)
            bursts[4 * n + (k % 8 if diagonal else k % 4)][j if j < 57 else j + 2] = block[k]
    return bursts


def remainder(bits):
    """the bits as a polynomial, first bit the highest power, modulo g: long division"""
    r = 0
    for b in bits:
        r = (r << 1) | b
        if r >> 40:
            r ^= G
    return r


def syndrome(bits):
    return remainder(bits) ^ ((1 << 40) - 1)


_single = None


def single_bit_syndromes():
    """the syndrome change an error in bit t alone makes, t = 0 .. 223"""
    global _single
    if _single is None:
        _single = [remainder([1 if i == t else 0 for i in range(224)]) for t in range(224)]
    return _single


_patterns = None


def patterns():
    """{syndrome change: (length, first bit, mask of the flipped bits counted from the first)} of EVERY error pattern that starts and ends
    with a flipped bit, of length 1 .. 12, at every position inside the 224 bits -- by the single-bit syndromes and linearity.  The header
    says they are 438 271 with distinct non-zero syndromes: asserted here, once"""
    global _patterns
    if _patterns is None:
        single, table, count = single_bit_syndromes(), {}, 0
        for t0 in range(224):
            for length in range(1, min(12, 224 - t0) + 1):
                inner = max(length - 2, 0)
                ends = single[t0] ^ (single[t0 + length - 1] if length > 1 else 0)
                x = [ends] * (1 << inner)
                for middle in range(1, 1 << inner):
                    low = (middle & -middle).bit_length() - 1
                    x[middle] = x[middle & (middle - 1)] ^ single[t0 + 1 + low]
                for middle, value in enumerate(x):
                    table[value] = (length, t0, 1 | (middle << 1) | (1 << (length - 1)))
                    count += 1
        assert count == len(table) == 438271 and 0 not in table
        _patterns = table
    return _patterns


def correct(bits, max_burst):
    """(status, first_bit, syndrome, bits) by definition: the one pattern of length <= max_burst, among all patterns at all positions,
    whose flip makes the syndrome zero -- or -1 and the bits as they came"""
    s = syndrome(bits)
    if s == 0:
        return 0, 0, s, list(bits)
    hit = patterns().get(s)
    if hit is None or hit[0] > max_burst:
        return -1, 0, s, list(bits)
    length, t0, mask = hit
    out = list(bits)
    for i in range(length):
        out[t0 + i] ^= (mask >> i) & 1
    return length, t0, s, out


def tchfs(u, class2, high, low):
    """(260 speech bits, parity syndrome, erasures) of the 185 decoded bits and the 78 class II values"""
    d = [0] * 260
    for k in range(91):
        d[2 * k], d[2 * k + 1] = u[k], u[184 - k]
    erased = 0
    for k in range(78):
        d[182 + k] = 1 if 2 * class2[k] > high + low else 0
        erased += 2 * class2[k] == high + low
    r = 0
    for b in d[:50] + [u[91], u[92], u[93]]:
        r = (r << 1) | b
        if r & 8:
            r ^= 0b1011
    return d, r ^ 7, erased
