"""An independent restatement of the IS-95A forward traffic channel rules of include/vit_hip.h for the tests: the block interleaver as the
array the standard draws (written by columns, rows permuted by bit reversal, read by rows) and never as the formula A(i); repetition and
combining as Python loops; the rate decision with fractions.Fraction.  Nothing here imports the package."""
from fractions import Fraction

STEPS = (192, 96, 48, 24)
INFO_BITS = (172, 80, 40, 16)


def interleave(s):
    """the transmit side: the 384 repeated symbols s -> the 384 sent ones.  s is written column by column into an array of 64 rows and 6
    columns, the rows are permuted by the reversal of their 6-bit number, and the array is read row by row"""
    assert len(s) == 384
    array = [[None] * 6 for _ in range(64)]
    for col in range(6):
        for row in range(64):
            array[row][col] = s[64 * col + row]
    permuted = [array[int(format(row, "06b")[::-1], 2)] for row in range(64)]
    return [x for row in permuted for x in row]


def deinterleave(symbols, scramble_bits=None, shift=0, lo=None, hi=None):
    """one frame: the 384 received ints (and 384 scramble bits, or None) -> the four lists of 2 S_h combined values"""
    y = [-v if scramble_bits is not None and scramble_bits[i] else v for i, v in enumerate(symbols)]
    where = interleave(list(range(384)))                          # sent symbol i is repeated symbol where[i]
    s = [None] * 384
    for i, a in enumerate(where):
        s[a] = y[i]
    out = []
    for h in range(4):
        r = 1 << h
        row = []
        for q in range(384 // r):
            total = 0
            for j in range(r):
                total += s[q * r + j]
            v = (total + ((1 << shift) >> 1)) >> shift            # Python's >> floors: the arithmetic shift
            if lo is not None:
                v = max(v, lo)
            if hi is not None:
                v = min(v, hi)
            row.append(v)
        out.append(row)
    return out


def decide(present, errors, compared, syndrome, max_num, den):
    """one frame -> (rate, info_bits, errors, compared); rate 4 where nothing passes"""
    best = None
    for h in range(4):
        if not present[h]:
            continue
        if h < 2 and syndrome[h] != 0:
            continue
        if compared[h] <= 0:
            continue
        ser = Fraction(errors[h], compared[h])
        if ser > Fraction(max_num[h], den):
            continue
        if best is None or ser < best[0]:
            best = (ser, h)
    if best is None:
        return (4, 0, 0, 0)
    h = best[1]
    return (h, INFO_BITS[h], errors[h], compared[h])


def crc_bit_serial(width, poly, init, bits):
    """the CRC of a list of bits, MSB-first, nothing reflected, no final XOR"""
    reg = init
    for b in bits:
        top = (reg >> (width - 1)) & 1
        reg = (reg << 1) & ((1 << width) - 1)
        if top ^ b:
            reg ^= poly
    return reg
