"""Many lockstep streams on one shared window grid (vit_hip_decode_streams, include/vit_hip.h) restated on the CPU checker, for the
streams tests.

The buffer holds n_streams segments of T steps, `pitch` = m W steps apart.  The uniform windows of ALL streams are windows of one
grid of stride W over the buffer: stream s's window i is grid window s m + i.  The m - n_u grid windows between the last uniform
window of stream s and window 0 of stream s + 1 straddle the two segments: these bridge windows are decoded like any other and
dropped.  (n_streams - 1) m + n_u grid windows are launched -- none behind the last stream's, and none at all when a stream has no
uniform window (n_u = 0) -- plus one remainder window per stream where the last window is longer.  What is kept and how it is
stitched is the rule of vit_hip_decode_stream per stream (tests/stream_reference.py).
"""
import numpy as np

from tests.stream_reference import BEGIN, END, default_extension, stream_invalid, stream_windows

BRIDGE = "bridge"


def streams_invalid(K, n_streams, pitch, T, W, head, tail, flags, out_pitch_bytes=None):
    """the argument rule: None, or why the arguments are rejected (the size limits of the launchers aside)"""
    why = stream_invalid(K, T, W, head, tail, flags)
    if why:
        return why
    if n_streams < 1:
        return "streams"
    if pitch < T:
        return "pitch"
    if pitch % W:
        return "grid"
    if out_pitch_bytes is not None:
        a = 0 if flags & BEGIN else head
        b = T - (K - 1) if flags & END else T - tail
        if out_pitch_bytes < (b - a + 7) // 8:
            return "out_pitch"
    return None


def uniform_windows(K, T, W, head, tail, flags):
    """n_u: how many of one stream's windows have head + W + tail steps (all of them, or all but the last)"""
    _, _, wins = stream_windows(K, T, W, head, tail, flags)
    return len(wins) if wins[-1][1] == head + W + tail else len(wins) - 1


def streams_windows(K, n_streams, pitch, T, W, head, tail, flags):
    """the launched windows, grid windows first: [(owner, i, first_step, steps)] with owner a stream index and i the window's index
    in that stream, or owner BRIDGE and i None; first_step in steps of the whole buffer"""
    why = streams_invalid(K, n_streams, pitch, T, W, head, tail, flags)
    if why:
        raise ValueError(why)
    m = pitch // W
    _, _, wins = stream_windows(K, T, W, head, tail, flags)
    n, n_u = len(wins), uniform_windows(K, T, W, head, tail, flags)
    out = []
    if n_u:
        for g in range((n_streams - 1) * m + n_u):
            s, i = divmod(g, m)
            out.append((s, i, g * W, head + W + tail) if i < n_u else (BRIDGE, None, g * W, head + W + tail))
    if n_u < n:
        for s in range(n_streams):
            out.append((s, n - 1, s * pitch + wins[-1][0], wins[-1][1]))
    return out


def streams_route_reference(oracle, code, ocfg, buf, n_streams, pitch, T, W=1024, head=None, tail=None, flags=BEGIN):
    """buf [(n_streams - 1) pitch + T (or more)][R] -> (bytes [n_streams][ceil(n_out/8)], n_out, windows decoded) by the
    ROUTE: every launched window decoded with the oracle's reset / update / chainback, bridge windows included, then the bridge
    windows dropped and each stream's windows stitched"""
    K, R = code.K, code.R
    head = default_extension(K) if head is None else head
    tail = default_extension(K) if tail is None else tail
    buf = np.ascontiguousarray(buf).reshape(-1, R)
    a, b, wins = stream_windows(K, T, W, head, tail, flags)
    n = len(wins)
    table = oracle.branch_table(K, R, code.G, ocfg.high, ocfg.low)
    N = 1 << (K - 1)
    bits = np.zeros((n_streams, b - a), dtype=np.uint8)
    decoded = 0
    for owner, i, first, steps in streams_windows(K, n_streams, pitch, T, W, head, tail, flags):
        assert first + steps <= buf.shape[0], "a launched window reads past the buffer"
        # a bridge window at a stream's grid position 0 cannot exist (position 0 is always the stream's window 0 when n_u > 0)
        if owner != BRIDGE and i == 0 and flags & BEGIN:
            metrics = oracle.reset(K, R, ocfg, 0)
        else:
            metrics = np.full(N, ocfg.initial_start_error, dtype=np.uint32)
        dec, _ = oracle.update(K, R, ocfg, table, metrics, buf[first:first + steps])
        end = 0 if owner != BRIDGE and i == n - 1 and flags & END else int(np.argmin(metrics))
        Lw = steps - (K - 1)
        wbits = np.unpackbits(oracle.chainback(K, dec, Lw, end))[:Lw]
        decoded += 1
        if owner == BRIDGE:
            continue                                          # decoded like any other, output dropped
        _, _, lo, hi = wins[i]
        rel = first - owner * pitch                           # the window's first step within its stream
        bits[owner, lo - a:hi - a] = wbits[lo - rel:hi - rel]
    return np.packbits(bits, axis=1, bitorder="big"), b - a, decoded
