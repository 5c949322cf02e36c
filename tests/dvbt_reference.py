"""An independent restatement of the DVB-T inner interleaver and puncturing (ETSI EN 300 744 clauses 4.3.3, 4.3.4) in the standard's own
direction, for the tests of viterbidecodercpp_amd/dvbt.py and the GPU call: the transmit-side scatter built literally -- puncture ->
demultiplex -> per-stream bit interleave -> symbol interleave, H generated bit by bit from lists of bits, no shifts -- over a stream of
labels, inverted by argsort.  Shares no code with dvbt.py."""
import functools

import numpy as np

MODES = {"2k": (2048, 1512, 11, [0, 3], [0, 7, 5, 1, 8, 2, 6, 9, 3, 4]),
         "4k": (4096, 3024, 12, [0, 2], [7, 10, 5, 8, 1, 2, 4, 9, 0, 3, 6]),
         "8k": (8192, 6048, 13, [0, 1, 4, 6], [5, 11, 3, 0, 10, 8, 6, 9, 2, 4, 1, 7])}
# what one period sends, in order; the package's output index of X is 1, of Y 0
SENT = [["X1", "Y1"], ["X1", "Y1", "Y2"], ["X1", "Y1", "Y2", "X3"], ["X1", "Y1", "Y2", "X3", "Y4", "X5"],
        ["X1", "Y1", "Y2", "Y3", "Y4", "X5", "Y6", "X7"]]
PERIOD = [1, 2, 3, 5, 7]
SHIFTS = [0, 63, 105, 42, 21, 84]


@functools.lru_cache(maxsize=None)
def h_table(mode):
    m_max, n_max, n_r, taps, wires = MODES[mode]
    word = [0] * (n_r - 1)                                          # word[b] = bit b of R'
    h = []
    for i in range(m_max):
        if i == 2:
            word = [1] + [0] * (n_r - 2)
        elif i > 2:
            new = sum(word[b] for b in taps) % 2
            word = word[1:] + [new]
        r_bits = [0] * (n_r - 1)
        for t, to in enumerate(wires):
            r_bits[to] = word[n_r - 2 - t]
        value = sum(bit * 2 ** b for b, bit in enumerate(r_bits)) + (i % 2) * 2 ** (n_r - 1)
        if value < n_max:
            h.append(value)
    return h


def steps_per_symbol(mode, v, rate):
    return MODES[mode][1] * v * PERIOD[rate] // (PERIOD[rate] + 1)


@functools.lru_cache(maxsize=None)
def scatter(mode, v, rate, odd):
    """for every element [carrier][e] of one transmitted OFDM symbol, the label 2 n + o of the mother-code bit it carries"""
    n_max = MODES[mode][1]
    h = h_table(mode)
    labels = []
    for n0 in range(0, steps_per_symbol(mode, v, rate), PERIOD[rate]):
        for name in SENT[rate]:
            labels.append(2 * (n0 + int(name[1]) - 1) + (1 if name[0] == "X" else 0))
    b = [[None] * n_max for _ in range(v)]
    for di, label in enumerate(labels):
        r = di % v
        b[r // (v // 2) + 2 * (r % (v // 2))][di // v] = label
    a = [[b[e][126 * (w // 126) + (w % 126 + SHIFTS[e]) % 126] for w in range(n_max)] for e in range(v)]
    sent = [None] * (n_max * v)
    for q in range(n_max):
        for e in range(v):
            if odd:
                sent[q * v + e] = a[e][h[q]]                        # y_q = y'_H(q)
            else:
                sent[h[q] * v + e] = a[e][q]                        # y_H(q) = y'_q
    return np.array(sent, dtype=np.int64)


def deinterleave(soft, mode, v, rate, parity=0):
    """soft [rows][n_sym][Nmax * v] -> [rows][n_sym * steps][2], 0 where nothing was sent; parity a scalar or one per row"""
    soft = np.asarray(soft)
    rows, n_sym = soft.shape[:2]
    steps = steps_per_symbol(mode, v, rate)
    first = np.broadcast_to(np.asarray(parity, dtype=np.int64), (rows,))
    out = np.zeros((rows, n_sym, 2 * steps), dtype=soft.dtype)
    for r in range(rows):
        for y in range(n_sym):
            labels = scatter(mode, v, rate, int(first[r] + y) % 2)
            order = np.argsort(labels)                              # element that carries the i-th smallest label
            out[r, y, labels[order]] = soft[r, y, order]
    return out.reshape(rows, n_sym * steps, 2)
