"""Overlapped-window decoding of one long stream restated on the CPU checker (oracle/viterbi_oracle.c), for the stream tests.

The rule of vit_hip_decode_stream (include/vit_hip.h), written in terms of the reference's reset / update / chainback: one call
decodes a segment of T steps; emitted range [a, b) with a = BEGIN ? 0 : head, b = END ? T-(K-1) : T-tail; n = max(1, (b-head)//W)
windows, window i over steps [i W, i W + head + W + tail), the last one over [(n-1) W, T); window 0 under BEGIN starts from
reset(0), every other one with every metric at initial_start_error; the last window under END ends in state 0, every other one in
the argmin of its final metrics (unsigned, lowest state on a tie); window i emits bits [head + i W, head + (i+1) W) of the segment
(window 0 under BEGIN from 0, the last one up to b) out of its chainback over steps - (K-1) bits.
"""
import numpy as np

from viterbidecodercpp_amd import synth

BEGIN, END = 1, 2
DEFAULT_WINDOW = 1024


def default_extension(K):
    return 8 * (K - 1)


def stream_invalid(K, T, W, head, tail, flags):
    """the argument rule: None, or why the arguments are rejected (the size limits of the launchers aside)"""
    if flags & ~(BEGIN | END):
        return "flags"
    if head < K - 1 or tail < K - 1:
        return "extension"
    if W < 8 or W < head or W < tail:
        return "window"
    if T < head + tail + (0 if flags & BEGIN else 1):
        return "short"
    a = 0 if flags & BEGIN else head
    b = T - (K - 1) if flags & END else T - tail
    if b <= a:
        return "empty"
    return None


def stream_windows(K, T, W, head, tail, flags):
    """(a, b, [(first_step, steps, emit_from, emit_to)]) -- the emitted bit ranges in steps of the segment"""
    why = stream_invalid(K, T, W, head, tail, flags)
    if why:
        raise ValueError(why)
    a = 0 if flags & BEGIN else head
    b = T - (K - 1) if flags & END else T - tail
    n = max(1, (b - head) // W)
    wins = []
    for i in range(n):
        last = i == n - 1
        first = i * W
        steps = T - first if last else head + W + tail
        lo = a if i == 0 else head + i * W
        hi = b if last else head + (i + 1) * W
        wins.append((first, steps, lo, hi))
    return a, b, wins


def stream_reference(oracle, code, ocfg, sym, W=DEFAULT_WINDOW, head=None, tail=None, flags=BEGIN):
    """sym [T][R] soft -> (bytes [ceil(n_out/8)] uint8 MSB-first with pad bits 0, n_out)"""
    K, R = code.K, code.R
    head = default_extension(K) if head is None else head
    tail = default_extension(K) if tail is None else tail
    sym = np.ascontiguousarray(sym).reshape(-1, R)
    T = sym.shape[0]
    a, b, wins = stream_windows(K, T, W, head, tail, flags)
    table = oracle.branch_table(K, R, code.G, ocfg.high, ocfg.low)
    N = 1 << (K - 1)
    bits = np.zeros(b - a, dtype=np.uint8)
    for i, (first, steps, lo, hi) in enumerate(wins):
        if i == 0 and flags & BEGIN:
            metrics = oracle.reset(K, R, ocfg, 0)
        else:
            metrics = np.full(N, ocfg.initial_start_error, dtype=np.uint32)
        dec, _ = oracle.update(K, R, ocfg, table, metrics, sym[first:first + steps])
        if i == len(wins) - 1 and flags & END:
            end = 0
        else:
            end = int(np.argmin(metrics))                  # first index of the minimum: the lowest state on a tie
        Lw = steps - (K - 1)
        wbits = np.unpackbits(oracle.chainback(K, dec, Lw, end))[:Lw]
        bits[lo - a:hi - a] = wbits[lo - first:hi - first]
    return np.packbits(bits, bitorder="big"), b - a


def full_decode(oracle, code, ocfg, sym):
    """the whole terminated stream sym [L+K-1][R] as ONE frame through the oracle: bits [L] uint8"""
    sym = np.ascontiguousarray(sym).reshape(-1, code.R)
    L = sym.shape[0] - (code.K - 1)
    out = oracle.decode(code.K, code.R, code.G, ocfg, sym, L)["bytes"]
    return np.unpackbits(out)[:L]


def make_stream(code, pc, L, ebn0, seed):
    """(info bits [L] uint8, symbols [L+K-1][R]) of one terminated stream through the AWGN quantiser; ebn0 None: noise-free"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=L, dtype=np.uint8)
    padded = np.concatenate([bits, np.zeros(code.K - 1, dtype=np.uint8)])
    reg = np.zeros(L + code.K - 1, dtype=np.int64)
    # state register at step t: the last K inputs, newest in bit 0
    for k in range(code.K):
        reg[k:] |= padded[:len(padded) - k].astype(np.int64) << k
    coded = np.zeros((L + code.K - 1, code.R), dtype=np.uint8)
    for i, g in enumerate(code.G):
        x = reg & int(g)
        par = np.zeros_like(x)
        for k in range(code.K):
            par ^= (x >> k) & 1
        coded[:, i] = par
    sym = synth.quantise_numpy(coded[None], pc.soft_decision_high, pc.soft_decision_low, ebn0, code.R, rng, pc.soft_dtype)[0]
    return bits, sym


def chunked_reference(oracle, code, ocfg, sym, seg_windows, W, head, tail):
    """the terminated stream sym [T][R] decoded as a chain of segments: segment j holds head + seg_windows[j] W + tail steps on the
    window grid (BEGIN on the first), the rest goes to the final END segment.  Returns (bits, n_bits)."""
    T = sym.shape[0]
    pos, out, first = 0, [], True
    for nw in seg_windows:
        seg = head + nw * W + tail
        assert pos + seg < T
        by, n = stream_reference(oracle, code, ocfg, sym[pos:pos + seg], W, head, tail, BEGIN if first else 0)
        out.append(np.unpackbits(by)[:n])
        pos += nw * W                                       # the next segment starts head + tail steps before this one's end
        first = False
    by, n = stream_reference(oracle, code, ocfg, sym[pos:], W, head, tail, (BEGIN if first else 0) | END)
    out.append(np.unpackbits(by)[:n])
    bits = np.concatenate(out)
    return bits, bits.size
