"""The rule of vit_hip_marker_search (include/vit_hip.h) written twice, independently of viterbidecodercpp_amd.frame_sync: a bit-by-bit
loop, and a vectorised form (64-bit windows, xor, popcount) for the larger cases; the pick on per-phase totals; and the makers of the
cases the CPU and GPU tests share."""
import numpy as np


def marker_bits_of(marker, m):
    return [(int(marker) >> (m - 1 - j)) & 1 for j in range(m)]


def stream_bits(row, n_bits, history, hb):
    """the hb history bits (the latest last) followed by the row's n_bits bits, MSB-first"""
    before = [(int(history) >> (hb - 1 - i)) & 1 for i in range(hb)]
    return np.concatenate([np.array(before, dtype=np.uint8), np.unpackbits(np.asarray(row, dtype=np.uint8))[:n_bits]])


def search_loop(rows, n_bits, marker, m, P, phase0=0, history=None, hb=0):
    """bit by bit: (distance, count) int64 [rows][P]"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.uint8))
    want = marker_bits_of(marker, m)
    distance = np.zeros((rows.shape[0], P), dtype=np.int64)
    count = np.zeros((rows.shape[0], P), dtype=np.int64)
    for r in range(rows.shape[0]):
        bits = stream_bits(rows[r], n_bits, 0 if history is None else history[r], hb)
        for p in range(-hb, n_bits - m + 1):
            phase = (phase0 + p) % P
            distance[r, phase] += sum(int(bits[p + hb + j]) != want[j] for j in range(m))
            count[r, phase] += 1
    return distance, count


def search_fast(rows, n_bits, marker, m, P, phase0=0, history=None, hb=0):
    """the same through 64-bit windows: shift the stream in one bit at a time, xor with the marker, count the ones"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.uint8))
    distance = np.zeros((rows.shape[0], P), dtype=np.int64)
    count = np.zeros((rows.shape[0], P), dtype=np.int64)
    n_pos = n_bits + hb - m + 1
    phase = (phase0 - hb + np.arange(n_pos, dtype=np.int64)) % P
    for r in range(rows.shape[0]):
        bits = stream_bits(rows[r], n_bits, 0 if history is None else history[r], hb).astype(np.uint64)
        window = np.zeros(n_pos, dtype=np.uint64)
        for j in range(m):
            window |= bits[j:j + n_pos] << np.uint64(m - 1 - j)
        x = window ^ np.uint64(marker)
        d = np.unpackbits(x.view(np.uint8).reshape(n_pos, 8), axis=1).sum(axis=1).astype(np.int64)
        np.add.at(distance[r], phase, d)
        np.add.at(count[r], phase, 1)
    return distance, count


def beats(ea, ca, eb, cb):
    return ca > 0 and (cb == 0 or ea * cb < eb * ca)


# a pair of rates one error apart whose 64-bit products differ by less than 2^32 and whose low halves order the other way: errors
# below half of compared, so that the upright candidates are the contenders
WRAP_COMPARED = 4_000_000_000
WRAP_ERRORS = next(e for e in range(1_000_000_000, 1_000_000_064)
                   if not (e * WRAP_COMPARED) & 0xFFFFFFFF < ((e + 1) * WRAP_COMPARED) & 0xFFFFFFFF)


def pick(distance, count, m):
    """[rows][4] int64 of (phase, inverted, errors, compared): the candidate no other beats, the lower (phase, inverted) on a tie.  The
    candidates are shortlisted by their rate in floating point (generously), then compared exactly in Python integers."""
    distance = np.atleast_2d(np.asarray(distance, dtype=np.int64))
    count = np.atleast_2d(np.asarray(count, dtype=np.int64))
    out = np.zeros((distance.shape[0], 4), dtype=np.int64)
    for r in range(distance.shape[0]):
        compared = np.repeat(m * count[r], 2)
        errors = np.stack([distance[r], m * count[r] - distance[r]], axis=1).reshape(-1)     # index 2 * phase + inverted
        live = np.flatnonzero(compared > 0)
        if live.size == 0:
            out[r] = (0, 0, int(errors[0]), 0)
            continue
        rate = errors[live] / compared[live]
        short = live[rate <= rate.min() * (1 + 1e-9) + 1e-12]
        best = int(short[0])
        for i in short[1:]:
            if beats(int(errors[i]), int(compared[i]), int(errors[best]), int(compared[best])):
                best = int(i)
        out[r] = (best // 2, best % 2, int(errors[best]), int(compared[best]))
    return out


def pick_loop(distance, count, m):
    """the pick as the header words it: every candidate in order, replaced only by one that beats it"""
    out = []
    for d_row, c_row in zip(np.atleast_2d(distance), np.atleast_2d(count)):
        best = None
        for phase in range(len(d_row)):
            compared = m * int(c_row[phase])
            for inverted, errors in ((0, int(d_row[phase])), (1, compared - int(d_row[phase]))):
                if best is None or beats(errors, compared, best[2], best[3]):
                    best = (phase, inverted, errors, compared)
        out.append(best)
    return np.array(out, dtype=np.int64)


def random_marker(rng, m):
    return int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2)) & ((1 << m) - 1)


def make_case(seed, rows, n_bits, m, P, hb=0, phase0=0, marker=None, stride_extra=0, plant=None):
    """a random case: `bytes` [rows][stride] uint8 (the pad bits of the last byte and the bytes behind it are random too: the rule
    never reads them as data), `history` [rows] uint64 or None.  plant = (phase, inverted): the marker (or its complement) is written
    at every position of that phase that lies wholly inside the row."""
    rng = np.random.default_rng(seed)
    nb = (n_bits + 7) // 8
    stride = nb + stride_extra
    marker = random_marker(rng, m) if marker is None else int(marker)
    data = rng.integers(0, 256, size=(rows, max(stride, 1)), dtype=np.uint8)[:, :stride]
    history = rng.integers(0, 1 << 63, size=rows, dtype=np.uint64) if hb else None
    if plant is not None:
        want = np.array(marker_bits_of(marker, m), dtype=np.uint8) ^ np.uint8(plant[1])
        for r in range(rows):
            bits = np.unpackbits(data[r, :nb])
            for p in range(0, n_bits - m + 1):
                if (phase0 + p) % P == plant[0]:
                    bits[p:p + m] = want
            data[r, :nb] = np.packbits(bits)
    return dict(bytes=data, n_bits=n_bits, marker=marker, m=m, P=P, hb=hb, phase0=phase0, history=history, rows=rows, stride=stride,
                nb=nb)


def case_reference(c, form=search_fast):
    """(distance, count, lock) of a case of make_case"""
    d, n = form(c["bytes"][:, :c["nb"]], c["n_bits"], c["marker"], c["m"], c["P"], c["phase0"], c["history"], c["hb"])
    return d, n, pick(d, n, c["m"])


def frames_with_marker(seed, marker, m, P, n_frames, phase, n_bits=None):
    """a bit stream (0/1 uint8) of random payload with the marker at every position of phase `phase` (mod P): n_frames periods"""
    rng = np.random.default_rng(seed)
    n_bits = n_frames * P if n_bits is None else n_bits
    bits = rng.integers(0, 2, size=n_bits, dtype=np.uint8)
    want = np.array(marker_bits_of(marker, m), dtype=np.uint8)
    for p in range(phase, n_bits - m + 1, P):
        bits[p:p + m] = want
    return bits
