"""vit_hip_depuncture_batch on the device, through the C ABI so that ANY map reaches the kernel, against three lines of numpy:
out[f, k] = inp[f, idx[k]] if 0 <= idx[k] < P else 0.  Every byte of a poisoned buffer around the output is compared; the shapes are
the smallest that tell the kernel's paths apart (a chunk of 8 symbols full or ragged, its store vector or scalar, one block or more);
maps that are no prefix sum; entries at or above punctured_per_frame, first where a kernel without the bound would read wrong values
inside the allocation, only then far away; every rejection with the output untouched; the call captured into a graph in front of the
decode; and a punctured rate the suite lacks (LTE to 1/2) end to end against the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, _lib, synth
from viterbidecodercpp_amd.codes import Code
from tests.helpers import make_table_config, oracle_cfg

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
WIDTHS = {2: "SOFT16", 1: "SOFT8"}
N_OUT = [1, 7, 8, 9, 15, 16, 17, 24, 1001]
FRAMES = [1, 2, 37, 300]                       # 300 frames x 126 chunks of 1001 symbols: more than one block of 256 threads
OFFSETS = [0, 1, 3, 8]                         # of the output's base from a 16-byte boundary, in elements
MAPS = ["prefix", "identity", "reversed", "repeated", "permuted", "erased", "negative"]


@functools.lru_cache(maxsize=None)
def handle(R, width):
    """(code, pc, decoder): a rate-1 generic code with K = 3 (any n_out is legal), Voyager (R = 2), LTE (R = 3)"""
    code = {1: Code("K3R1", 3, 1, (0o7,)), 2: COMMON_CODES[2], 3: COMMON_CODES[3]}[R]
    pc, table, config = make_table_config(code, WIDTHS[width])
    return code, pc, (BatchDecoder(table, config, plan=_lib.PLAN_LDS) if R == 1 else BatchDecoder(table, config))


def reference(inp, idx, P):
    ok = (idx >= 0) & (idx < P)
    out = np.zeros((inp.shape[0], idx.size), dtype=inp.dtype)
    out[:, ok] = inp[:, idx[ok]]
    return out


def make_map(kind, n_out, P, rng):
    """int32 [n_out]; every non-negative entry lies below P (the out-of-range entries have a test of their own)"""
    k = np.arange(n_out)
    if P == 0 or kind == "erased":
        idx = np.full(n_out, -1)
    elif kind == "prefix":
        mask = rng.random(n_out) < 0.6
        idx = np.where(mask & (np.cumsum(mask) <= P), np.cumsum(mask) - 1, -1)
    elif kind == "identity":
        idx = k % P
    elif kind == "reversed":
        idx = (n_out - 1 - k) % P
    elif kind == "repeated":
        idx = np.full(n_out, rng.integers(0, P))
    elif kind == "permuted":
        idx = rng.permutation(P)[:n_out] if P >= n_out else rng.integers(0, P, n_out)
        idx = np.where(rng.random(n_out) < 0.3, -1, idx)
    else:                                       # negative values other than -1
        idx = rng.choice(np.array([INT32_MIN, INT32_MIN + 1, -(1 << 30), -65536, -7, -2]), n_out)
        idx[rng.random(n_out) < 0.3] = rng.integers(0, P)
    return idx.astype(np.int32)


def symbols(rng, shape, dtype):
    """random over the whole type, never 0: a gathered symbol differs from an erasure"""
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max + 1, shape).astype(dtype)
    x[x == 0] = 1
    return x


def run(width, R, inp, idx, frames, off=0, tail=0, n_out=None):
    """one call with the output `off` elements behind a 16-byte boundary inside a poisoned buffer, GUARD elements in front and behind;
    the input ends with its allocation, or `tail` elements of 0x5A in front of that.  Returns (code, whole buffer, expected buffer)"""
    import torch
    dt = {2: torch.int16, 1: torch.int8}[width]
    npdt = inp.dtype
    n_out = idx.size if n_out is None else n_out
    P = inp.shape[1]
    poison = np.frombuffer(bytes([POISON] * width), dtype=npdt)[0]
    lead = 1 if inp.size + tail == 0 else 0                       # a pointer that is not NULL where the input has no element
    flat = np.concatenate([np.zeros(lead, npdt), inp.reshape(-1), np.frombuffer(bytes([0x5A] * (width * tail)), dtype=npdt)])
    d_in = torch.from_numpy(flat).cuda()
    d_idx = torch.from_numpy(idx).cuda()
    buf = torch.full((GUARD + off + frames * n_out + GUARD,), int(poison), dtype=dt, device="cuda")
    assert buf.data_ptr() % 16 == 0 and (GUARD * width) % 16 == 0
    at = GUARD + off
    rc = _lib.load().vit_hip_depuncture_batch(handle(R, width)[2]._handle._h, d_in.data_ptr() + lead * width, P, d_idx.data_ptr(), n_out, frames,
                                              buf.data_ptr() + at * width, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    want = np.full(buf.numel(), poison, dtype=npdt)
    want[at:at + frames * n_out] = reference(inp, idx.astype(np.int64), P).reshape(-1)
    return rc, buf.cpu().numpy(), want


def check(width, R, n_out, frames, P, off, kind, seed):
    rng = np.random.default_rng(seed)
    dtype = {2: np.int16, 1: np.int8}[width]
    inp = symbols(rng, (frames, P), dtype)
    idx = make_map(kind, n_out, P, rng)
    rc, got, want = run(width, R, inp, idx, frames, off)
    tag = dict(width=width, R=R, n_out=n_out, frames=frames, P=P, off=off, map=kind)
    assert rc == _lib.OK, (tag, _lib.load().vit_hip_last_error())
    assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("n_out", N_OUT)
@pytest.mark.parametrize("width", [2, 1])
def test_every_shape_at_rate_1(width, n_out):
    """the full cross product frames x P x output offset at one n_out; the maps cycle beside it (96 calls, 7 kinds)"""
    i = 0
    for frames in FRAMES:
        for P in sorted({0, 1, 2, 13, n_out, 2 * n_out}):
            for off in OFFSETS:
                check(width, 1, n_out, frames, P, off, MAPS[i % len(MAPS)], 100000 * width + 100 * n_out + i)
                i += 1


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("width", [2, 1])
def test_every_map_at_rates_2_and_3(width, R):
    """the multiples of R next to the n_out of rate 1, every map at each; frames, P and the offset cycle beside them"""
    sizes = sorted({m for n in N_OUT for m in (n // R * R, -(-n // R) * R) if m > 0})
    i = 0
    for n_out in sizes:
        for kind in MAPS:
            frames = FRAMES[i % 4] if n_out < 900 else (1, 2, 37)[i % 3]
            P = (0, 1, 2, 13, n_out, 2 * n_out)[(i // 2) % 6]
            check(width, R, n_out, frames, P, OFFSETS[(i // 3) % 4], kind, 7000 * R + 1000000 * width + i)
            i += 1


@pytest.mark.parametrize("width", [2, 1])
def test_out_of_range_entries_read_as_erasures(width):
    """entries at or above punctured_per_frame.  Step one: indices in [P, P + 32] with 64 elements of 0x5A behind the last frame, so
    that a kernel WITHOUT the bound reads wrong values (the next frame's symbols, the poison) yet touches nothing outside the
    allocation: it fails here by comparison.  Only when all of step one holds, step two: INT32_MAX and 2^30, the input ending with
    its allocation."""
    dtype = {2: np.int16, 1: np.int8}[width]
    rng = np.random.default_rng(50 + width)
    shapes = [(R, n_out, frames, P) for i, (R, n_out) in enumerate([(1, 9), (1, 24), (1, 1001), (2, 16), (3, 9), (1, 17)])
              for frames in (1, 2, 37) for P in sorted({0, 1, 2, 13, n_out, 2 * n_out})]
    for step in (1, 2):
        for j, (R, n_out, frames, P) in enumerate(shapes):
            inp = symbols(rng, (frames, P), dtype)
            far = rng.integers(P, P + 33, n_out) if step == 1 else rng.choice(np.array([INT32_MAX, 1 << 30, INT32_MAX - 1]), n_out)
            inside = rng.random(n_out) < 0.4                   # in-range entries between them: the frame is still gathered right
            idx = np.where(inside & (P > 0), rng.integers(0, max(P, 1), n_out), far).astype(np.int32)
            idx[0] = far[0]
            rc, got, want = run(width, R, inp, idx, frames, OFFSETS[j % 4], tail=64 if step == 1 else 0)
            tag = dict(step=step, R=R, n_out=n_out, frames=frames, P=P)
            assert rc == _lib.OK, tag
            assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:4].tolist())
            out = got[GUARD + OFFSETS[j % 4]:][:frames * n_out].reshape(frames, n_out)
            assert (out[:, idx >= P] == 0).all(), tag          # no symbol of the next frame, no poison leaks in


class Arena:
    """one byte buffer [guard][out A][input][pad][map][out B][guard]: A ends where the input begins, B begins where the map ends"""

    def __init__(self, width, n_out, frames, P, seed):
        import torch
        rng = np.random.default_rng(seed)
        self.width, self.n_out, self.frames, self.P = width, n_out, frames, P
        self.dtype = {2: np.int16, 1: np.int8}[width]
        self.inp = symbols(rng, (frames, P), self.dtype)
        self.idx = make_map("permuted", n_out, P, rng)
        O, I = frames * n_out * width, frames * P * width
        self.a = GUARD
        self.i = self.a + O
        self.m = (self.i + I + 3) // 4 * 4
        self.b = self.m + 4 * n_out
        self.image = np.full(self.b + O + GUARD, POISON, dtype=np.uint8)
        self.image[self.i:self.i + I] = self.inp.reshape(-1).view(np.uint8)
        self.image[self.m:self.b] = self.idx.view(np.uint8)
        self.O = O
        self.buf = torch.from_numpy(self.image.copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def call(self, h="h", d_in="i", d_idx="m", d_out="a", n_out=None, frames=None, R=1, bump=(0, 0, 0)):
        import torch
        base = self.buf.data_ptr()
        at = lambda name, plus: None if name is None else base + getattr(self, name) + plus          # noqa: E731
        rc = _lib.load().vit_hip_depuncture_batch(
            None if h is None else handle(R, self.width)[2]._handle._h, at(d_in, bump[0]), self.P, at(d_idx, bump[1]),
            self.n_out if n_out is None else n_out, self.frames if frames is None else frames, at(d_out, bump[2]),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return np.array_equal(self.buf.cpu().numpy(), self.image)


@pytest.mark.parametrize("width", [2, 1])
def test_rejections_launch_nothing(width):
    """every rejected call returns VIT_HIP_ERR_INVALID_ARG and leaves every byte as it was; frames = 0 and symbols_per_frame = 0 are
    no work and no error; then one call at each of the two tight bounds passes and does write"""
    ar = Arena(width, 24, 3, 13, seed=9 + width)
    BAD = _lib.ERR_INVALID_ARG
    last = lambda: _lib.load().vit_hip_last_error()                                    # noqa: E731
    cases = [
        (dict(h=None), b"NULL handle"), (dict(d_in=None), b"NULL buffer"), (dict(d_idx=None), b"NULL buffer"), (dict(d_out=None), b"NULL buffer"),
        (dict(R=2, n_out=23), b"multiple of the code rate"), (dict(R=3, n_out=23), b"multiple of the code rate"),
        (dict(bump=(0, 2, 0)), b"d_source_index must be aligned"), (dict(bump=(0, 1, 0)), b"d_source_index must be aligned"),
        (dict(bump=(0, 3, 0)), b"d_source_index must be aligned"),
        # the output on the input's first and on its last element; inside the map, and on the map's last bytes
        (dict(d_out="i", bump=(0, 0, width - ar.O)), b"overlaps d_punctured"), (dict(d_out="i", bump=(0, 0, ar.frames * ar.P * width - width)), b"overlaps d_punctured"),
        (dict(d_out="i"), b"overlaps d_punctured"),
        (dict(d_out="m"), b"overlaps d_source_index"), (dict(d_out="b", bump=(0, 0, -width)), b"overlaps d_source_index"),
        (dict(frames=1 << 40, n_out=8), b"too large for one launch"),
    ]
    if width == 2:
        cases += [(dict(bump=(1, 0, 0)), b"aligned to the symbol type"), (dict(bump=(0, 0, 1)), b"aligned to the symbol type")]
    for kw, why in cases:
        assert ar.call(**kw) == BAD and why in last(), (kw, last())
        assert ar.untouched(), kw
    for kw in (dict(frames=0), dict(n_out=0), dict(frames=0, d_in=None, d_idx=None, d_out=None)):
        assert ar.call(**kw) == _lib.OK, kw
        assert ar.untouched(), kw
    want = reference(ar.inp, ar.idx.astype(np.int64), ar.P).reshape(-1).view(np.uint8)
    for slot in ("a", "b"):
        assert ar.call(d_out=slot) == _lib.OK, (slot, last())
        at = getattr(ar, slot)
        ar.image[at:at + ar.O] = want
        assert not np.all(want == POISON) and ar.untouched(), slot


@pytest.mark.parametrize("width", [2, 1])
def test_depuncture_and_decode_captured_into_a_graph(oracle, width):
    """depuncture -> decode_batch on one stream, one chain: captured once, replayed on two inputs, each bit-exact against the oracle
    fed the host-depunctured symbols"""
    import torch
    code, pc, dec = handle(2, width)
    decode_type = WIDTHS[width]
    F, L = 37, 96
    S = L + code.K - 1
    mask = np.tile(np.array([1, 1, 0, 1, 1, 0], dtype=bool), S * code.R // 6)          # rate 1/2 punctured to 3/4
    P = int(mask.sum())
    d_in = torch.zeros((F, P), dtype=torch.int16 if width == 2 else torch.int8, device="cuda")
    d_sym = torch.empty((F, S, code.R), dtype=d_in.dtype, device="cuda")
    out = torch.empty((F, L // 8), dtype=torch.uint8, device="cuda")

    def chain():
        dec.depuncture(d_in, mask, out=d_sym)
        dec.decode(d_sym, L, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                    # warm-up outside the capture: the map is uploaded here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for seed, ebn0 in ((61, 5.0), (62, 7.0)):
        _, sym = synth.make_frames_numpy(code, pc, F, L, ebn0, seed=seed)
        sent = np.ascontiguousarray(sym.reshape(F, -1)[:, mask])
        d_in.copy_(torch.from_numpy(sent))
        d_sym.view(torch.uint8).fill_(POISON), out.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        host = np.zeros((F, mask.size), dtype=sym.dtype)
        host[:, mask] = sent
        assert np.array_equal(d_sym.cpu().numpy().reshape(F, -1), host)
        want, _, _ = oracle.decode_frames(code.K, code.R, code.G, oracle_cfg(decode_type, code.R), host, L)
        assert np.array_equal(out.cpu().numpy(), want), seed


@pytest.mark.parametrize("width", [2, 1])
def test_lte_punctured_to_rate_one_half_end_to_end(oracle, width):
    """LTE (K = 7, R = 1/3) punctured to 1/2 with a 6-symbol period (two steps send 4 of 6): 11 frames of L = 64, depunctured on the
    device and decoded; every frame equals the oracle on the host-depunctured stream, which itself decodes to the sent bytes at this
    noise"""
    import torch
    code, pc, dec = handle(3, width)
    decode_type = WIDTHS[width]
    F, L = 11, 64
    S = L + code.K - 1
    mask = np.tile(np.array([1, 1, 0, 1, 0, 1], dtype=bool), S * code.R // 6)
    assert mask.size == S * code.R and mask.sum() * 2 == S * 4
    tx, sym = synth.make_frames_numpy(code, pc, F, L, 8.0, seed=71)
    sent = np.ascontiguousarray(sym.reshape(F, -1)[:, mask])
    d_sym = dec.depuncture(torch.from_numpy(sent).cuda(), mask)
    host = np.zeros((F, mask.size), dtype=sym.dtype)
    host[:, mask] = sent
    assert np.array_equal(d_sym.cpu().numpy().reshape(F, -1), host)
    got = dec.decode(d_sym, L).cpu().numpy()
    for f in range(F):
        want = oracle.decode(code.K, code.R, code.G, oracle_cfg(decode_type, code.R), host[f], L)["bytes"]
        assert np.array_equal(got[f], want), f
    assert np.array_equal(got, tx) or width == 1              # SOFT16 at 8 dB: the punctured code still corrects everything
