"""Many lockstep streams on one shared window grid without a GPU: the C ABI, ctypes, Python and C++ surfaces exist, the grid
bookkeeping launches exactly the windows of every stream plus the bridge windows between them and stays inside the buffer, the
argument rule, and the route -- decode every grid window, drop the bridge windows, stitch -- restated on the CPU checker gives per
stream exactly the bits of the single-stream rule (tests/stream_reference.py)."""
import os
import subprocess

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, _lib, get_decoding_config

from tests.helpers import oracle_cfg
from tests.stream_reference import BEGIN, END, default_extension, make_stream, stream_invalid, stream_reference, stream_windows
from tests.streams_reference import BRIDGE, streams_invalid, streams_route_reference, streams_windows, uniform_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS_SYMBOLS = ["vit_hip_streams_workspace_bytes", "vit_hip_decode_streams"]


def test_streams_exports():
    lib = _lib.load()
    for name in STREAMS_SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert lib.vit_hip_streams_workspace_bytes.argtypes is not None and len(lib.vit_hip_streams_workspace_bytes.argtypes) == 8
    assert lib.vit_hip_decode_streams.argtypes is not None and len(lib.vit_hip_decode_streams.argtypes) == 15
    import viterbidecodercpp_amd
    from viterbidecodercpp_amd import BatchDecoder, MultiStreamDecoder
    assert "MultiStreamDecoder" in viterbidecodercpp_amd.__all__
    assert callable(BatchDecoder.decode_streams) and callable(BatchDecoder.streams_workspace_bytes)
    assert callable(MultiStreamDecoder.push) and callable(MultiStreamDecoder.finish)


def test_streams_cpp_surface(tmp_path):
    src = tmp_path / "streams.cpp"
    src.write_text(
        '#include "viterbi_hip/viterbi_decoder_hip_batch.h"\n'
        "size_t f(ViterbiDecoder_HIP_Batch<7, 2, uint16_t, int16_t>& d, const int16_t* sym, void* ws, uint8_t* out) {\n"
        "    const size_t n = d.streams_workspace_bytes(64, 17 * 1024, 48 + 16 * 1024 + 48, true, false);\n"
        "    size_t bits = d.decode_streams(sym, 64, 17 * 1024, 48 + 16 * 1024 + 48, true, false, ws, n, out, 2064);\n"
        "    bits += d.decode_streams(sym, 3, 40 * 129, 5000, false, true, ws, d.streams_workspace_bytes(3, 40 * 129, 5000, false, true, 129, 13, 19),\n"
        "                             out, 640, 129, 13, 19, nullptr);\n"
        "    return bits;\n"
        "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def _random_arguments(rng, K):
    """(n_streams, pitch, T, W, head, tail, flags) inside the argument rule, small values and edge cases over-represented"""
    while True:
        head = K - 1 + int(rng.integers(0, 3) * rng.integers(0, 20))
        tail = K - 1 + int(rng.integers(0, 3) * rng.integers(0, 20))
        W = max(8, head, tail) + int(rng.integers(0, 2) * rng.integers(0, 70))
        flags = int(rng.integers(0, 4))
        # segments of head + n W + tail steps (what the docs recommend), and anything else
        if rng.integers(0, 2):
            T = head + int(rng.integers(1, 7)) * W + tail
        else:
            T = head + tail + int(rng.integers(0, 3) * rng.integers(0, 6 * W)) + int(rng.integers(0, 3))
        if stream_invalid(K, T, W, head, tail, flags) is not None:
            continue
        pitch = -(-T // W) * W + int(rng.integers(0, 2) * rng.integers(0, 4)) * W       # minimal, or up to three windows more
        return int(rng.integers(1, 7)), pitch, T, W, head, tail, flags


def test_grid_bookkeeping():
    rng = np.random.default_rng(21)
    seen_uniform = seen_remainder = seen_no_grid = seen_two_bridges = 0
    for trial in range(4000):
        K = int(rng.integers(2, 17))
        ns, pitch, T, W, head, tail, flags = _random_arguments(rng, K)
        assert streams_invalid(K, ns, pitch, T, W, head, tail, flags) is None
        m = pitch // W
        _, _, one = stream_windows(K, T, W, head, tail, flags)
        n, n_u = len(one), uniform_windows(K, T, W, head, tail, flags)
        wins = streams_windows(K, ns, pitch, T, W, head, tail, flags)
        # the non-bridge windows of stream s are exactly the single-stream windows shifted by s * pitch
        for s in range(ns):
            mine = sorted((i, first, steps) for owner, i, first, steps in wins if owner == s)
            assert mine == [(i, s * pitch + first, steps) for i, (first, steps, _, _) in enumerate(one)], (trial, s)
        # every launched window lies inside the buffer, whose last stream holds T steps only
        for owner, i, first, steps in wins:
            assert 0 <= first and first + steps <= (ns - 1) * pitch + T, (trial, owner, i)
        # the grid: stride W, uniform length, (n_streams - 1) m + n_u windows; nothing on it when no stream has a uniform window
        grid = [w for w in wins if w[3] == head + W + tail and (w[0] == BRIDGE or w[1] < n_u)]
        rest = [w for w in wins if w not in grid]
        assert len(grid) == ((ns - 1) * m + n_u if n_u else 0)
        assert [w[2] for w in grid] == [g * W for g in range(len(grid))]
        assert sum(w[0] == BRIDGE for w in grid) == ((ns - 1) * (m - n_u) if n_u else 0)
        assert len(rest) == (ns if n_u < n else 0) and all(w[0] != BRIDGE for w in rest)
        assert len(wins) == len(grid) + len(rest)
        assert m >= n and m > n_u, "a stream's windows end inside its pitch"
        if not flags & END and T == head + n * W + tail and pitch == -(-T // W) * W:
            assert n_u == n and m == (n + 2 if head + tail > W else n + 1), "the smallest pitch of a uniform segment"
            seen_two_bridges += m == n + 2
        seen_uniform += n_u == n
        seen_remainder += 0 < n_u < n
        seen_no_grid += n_u == 0
    assert min(seen_uniform, seen_remainder, seen_no_grid, seen_two_bridges) > 50


def test_streams_argument_rule():
    K = 7
    ok = dict(n_streams=3, pitch=80 * 64, T=5000, W=64, head=6, tail=6, flags=BEGIN, out_pitch_bytes=(5000 - 6 + 7) // 8)
    assert streams_invalid(K, **ok) is None
    # everything vit_hip_decode_stream demands
    for change in (dict(head=5), dict(tail=5), dict(W=7, pitch=5005), dict(W=40, head=41, pitch=5000), dict(W=40, tail=41, pitch=5000),
                   dict(flags=4), dict(flags=BEGIN | 8), dict(T=11), dict(T=12, flags=0), dict(T=12, flags=END)):
        assert streams_invalid(K, **dict(ok, **change)) is not None, change
    # and the grid's own
    for change in (dict(n_streams=0), dict(pitch=78 * 64), dict(pitch=4999), dict(pitch=80 * 64 + 1), dict(pitch=5000),
                   dict(out_pitch_bytes=(5000 - 6 + 7) // 8 - 1)):
        assert streams_invalid(K, **dict(ok, **change)) is not None, change
    assert streams_invalid(K, **dict(ok, n_streams=1)) is None
    assert streams_invalid(K, **dict(ok, pitch=79 * 64)) is None              # 5056 >= 5000: the smallest pitch
    assert streams_invalid(K, **dict(ok, T=80 * 64, out_pitch_bytes=640)) is None   # pitch == T
    assert streams_invalid(K, **dict(ok, out_pitch_bytes=4096)) is None


ROUTE_SETS = [(2, "SOFT16"), (3, "SOFT8"), (5, "SOFT16"), (2, "HARD8")]


@pytest.mark.parametrize("code_id,decode_type", ROUTE_SETS)
def test_route_is_exact_on_the_cpu_checker(oracle, code_id, decode_type):
    """all grid windows of the concatenated buffer through the oracle's reset / update / chainback, random symbols in the padding,
    bridge windows dropped, the rest stitched: per stream the bytes of stream_reference on that stream alone"""
    code = COMMON_CODES[code_id]
    pc = get_decoding_config(decode_type, code.R)
    ocfg = oracle_cfg(decode_type, code.R)
    K, d = code.K, default_extension(code.K)
    W = max(64, d)
    rng = np.random.default_rng(100 + code_id)
    # (T, W, head, tail, extra windows of pitch): uniform, a longer last window, and head + tail > W (two bridge windows at least)
    shapes = [(d + 3 * W + d, W, d, d, 0), (d + 2 * W + d + 29, W, d, d, 1), (d + d + 9, W, d, d, 0),
              ((K + 30) + 3 * (K + 37) + (K + 20), K + 37, K + 30, K + 20, 0)]
    assert shapes[-1][2] + shapes[-1][3] > shapes[-1][1]
    # noisy, near 2.5 dB (hard decisions need more to leave the decoder something to do than to drown it)
    ebn0 = 4.0 if decode_type == "HARD8" else 2.5
    checked = 0
    for T, W, head, tail, extra in shapes:
        pitch = (-(-T // W) + extra) * W
        for ns in (1, 2, 5):
            for flags in (0, BEGIN, END, BEGIN | END):
                buf = np.empty(((ns - 1) * pitch + T, code.R), dtype=pc.soft_dtype)
                info = np.iinfo(buf.dtype)
                lo, hi = (0, 2) if decode_type == "HARD8" else (info.min // 2, info.max // 2)
                buf[:] = rng.integers(lo, hi, size=buf.shape)             # the padding between T and pitch: random symbols
                streams = []
                for s in range(ns):
                    _, sym = make_stream(code, pc, T + 50, ebn0, seed=1000 * code_id + 10 * checked + s)
                    first = 0 if flags & BEGIN else 13 + s
                    streams.append(sym[first:first + T])
                    buf[s * pitch:s * pitch + T] = streams[-1]
                got, n_out, decoded = streams_route_reference(oracle, code, ocfg, buf, ns, pitch, T, W, head, tail, flags)
                assert decoded == len(streams_windows(K, ns, pitch, T, W, head, tail, flags))
                for s in range(ns):
                    want, want_n = stream_reference(oracle, code, ocfg, streams[s], W, head, tail, flags)
                    assert n_out == want_n
                    assert np.array_equal(got[s], want), (code.name, decode_type, T, W, head, tail, ns, flags, s)
                checked += 1
    assert checked == len(shapes) * 3 * 4
