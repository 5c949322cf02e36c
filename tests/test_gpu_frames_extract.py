"""vit_hip_frames_extract on the device against tests/frames_reference.py: every byte of every output buffer -- written or not, the
guard bands around them included -- EQUAL to the image the rule gives, for the periods, lengths, carries, skips, drops, markers, pads,
polarities, row counts, odd addresses and odd strides the kernel tells apart; wild locks and carry lengths; every rejection with the
outputs untouched; cut invariance over 5 calls with ping-ponged carries; marker_search and frames_extract captured into one graph; and
the receivers' take_frames() against the numpy composition and the transmitted frames."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import CCSDS_ASM, COMMON_CODES, BatchDecoder, MultiStreamDecoder, StreamDecoder, _lib, frame_sync
from tests import frames_reference as fr
from tests.helpers import make_table_config
from tests.test_frames_cpu import FIRST_GOOD_FRAME, RECEIVER

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64


@functools.lru_cache(maxsize=None)
def decoder():
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    return code, pc, BatchDecoder(table, config)


def ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def placed(arr, stride, width, off):
    """the rows of arr [rows][>= width] on the device `stride` bytes apart, the first `off` bytes into an allocation that ends with the
    last row's last byte: a uint8 tensor that starts at row 0"""
    import torch
    rows = arr.shape[0]
    flat = np.full(off + (rows - 1) * stride + max(width, 1), 0xEE, dtype=np.uint8)
    for r in range(rows):
        n = min(stride, flat.size - off - r * stride, arr.shape[1])
        flat[off + r * stride: off + r * stride + n] = arr[r, :n]
    return torch.from_numpy(flat).cuda()[off:]


class Outputs:
    """the five outputs as slices of two poisoned buffers (bytes at odd offsets, words), with guard bands between them"""

    def __init__(self, c, off=0):
        import torch
        sizes = [c["rows"] * c["max_frames"] * c["fstride"], c["rows"] * c["cstride"]]
        self.bytes = torch.full((sum(sizes) + 3 * GUARD + 2 * off,), POISON, dtype=torch.uint8, device="cuda")
        at = GUARD + off
        self.frames = self.bytes[at:at + sizes[0]]
        at += sizes[0] + GUARD + off
        self.carry = self.bytes[at:at + sizes[1]]
        words = [c["rows"], c["rows"] * c["max_frames"], c["rows"]]
        self.words = torch.full((sum(words) + 4 * GUARD,), POISON * 0x01010101 - (1 << 32), dtype=torch.int32, device="cuda")
        at, parts = GUARD, []
        for n in words:
            parts.append(self.words[at:at + n])
            at += n + GUARD
        self.n, self.errors, self.carry_bits = parts
        self.off, self.sizes, self.nwords = off, sizes, words

    def expect(self, images):
        """the whole of both buffers as they must read after the call"""
        frames, n, errors, carry, bits = images
        b = np.full(self.bytes.numel(), POISON, dtype=np.uint8)
        at = GUARD + self.off
        b[at:at + self.sizes[0]] = frames
        at += self.sizes[0] + GUARD + self.off
        b[at:at + self.sizes[1]] = carry
        w = np.full(self.words.numel(), POISON * 0x01010101, dtype=np.uint32)
        at = GUARD
        for part in (n, errors, bits):
            w[at:at + part.size] = part
            at += part.size + GUARD
        return b, w

    def read(self):
        return self.bytes.cpu().numpy(), self.words.cpu().numpy().view(np.uint32)


def call(c, out, off=0, carry=True, errors=True, lock=None):
    import torch
    code, pc, dec = decoder()
    d_bytes = placed(c["bytes"], c["stride"], c["nb"], off)
    d_carry = placed(c["carry"], c["cstride"], c["cb"], off) if carry and c["carry"] is not None else None
    d_cbits = torch.from_numpy(c["carry_bits"].astype(np.uint32).view(np.int32)).cuda()
    d_lock = torch.from_numpy((c["lock"] if lock is None else lock).astype(np.uint32).view(np.int32)).cuda()
    d_pad = None if c["pad"] is None else placed(c["pad"][None], c["qb"], c["qb"], off)
    rc = _lib.load().vit_hip_frames_extract(
        dec._handle._h, ptr(d_bytes), c["stride"], c["rows"], c["n_bits"], c["P"], c["phase0"], ptr(d_lock), ptr(d_carry), ptr(d_cbits),
        c["cstride"], c["marker"], c["m"], c["d"], ptr(d_pad), ptr(out.frames), c["fstride"], c["max_frames"], ptr(out.n),
        ptr(out.errors) if errors else None, ptr(out.carry), ptr(out.carry_bits), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def check(c, off=0, errors=True):
    out = Outputs(c, off)
    assert call(c, out, off, errors=errors) == _lib.OK
    ref = fr.case_reference(c)
    if not errors:
        ref = [(f, None, co, rem) for f, _, co, rem in ref]
    want_b, want_w = out.expect(fr.images(c, ref, POISON))
    got_b, got_w = out.read()
    tag = {k: c[k] for k in ("rows", "n_bits", "P", "phase0", "d", "m", "stride", "cstride", "fstride", "max_frames")} | {"off": off}
    tag["c"], tag["lock"] = c["carry_bits"].tolist()[:3], c["lock"][:3, :2].tolist()
    assert np.array_equal(got_w, want_w), (tag, np.argwhere(got_w != want_w)[:4].tolist())
    assert np.array_equal(got_b, want_b), (tag, np.argwhere(got_b != want_b)[:4].tolist())
    return ref


PERIODS = [8, 13, 67, 83, 1632, 10232]          # 83 = 8 * 10 + 3


@pytest.mark.parametrize("P", PERIODS)
def test_periods_lengths_carries_and_skips(P):
    """n_bits in {1, P-1, P, 3P+5} x c in {0, 1, 7, 8, 9, P-1} x skip in {0, 1, P-1, >= total}; drop, marker length, pad, polarity, rows,
    base address and strides cycle through their values beside them"""
    i = 0
    for n_bits in (1, P - 1, P, 3 * P + 5):
        for c in (0, 1, 7, 8, 9, P - 1):
            c = min(c, P - 1)
            for skip in (0, 1, P - 1, "past"):
                if skip == "past":
                    skip = min(c + n_bits, P - 1)       # skip >= total where the call is shorter than a period, else the largest
                d = (0, 5, 32)[i % 3] % P
                m = min((0, 8, 32, 64)[(i // 3) % 4], P)
                rows = (1, 3, 64)[(i // 2) % 3] if P < 1000 or n_bits < P else (1, 3)[i % 2]
                case = fr.make_case(1000 * P + i, rows=rows, n_bits=n_bits, P=P, phase0=(0, 1, P - 1, P // 2)[i % 4], c=c, skip=skip,
                                    inverted=i % 2, d=d, m=m, pad=bool((i // 2) % 2), stride_extra=(0, 1, 2)[i % 3],
                                    carry_extra=(0, 1)[(i // 3) % 2], frame_extra=(0, 1, 3)[(i // 2) % 3], max_extra=(0, 2)[(i // 4) % 2],
                                    phase_plus=(0, P)[(i // 5) % 2])
                check(case, off=(1, 0, 3, 5)[i % 4])
                i += 1


@pytest.mark.parametrize("P,d,m", [(1632, 8, 8), (10232, 32, 32)])
def test_forty_periods(P, d, m):
    """many blocks, frames whose words lie on every bit offset, the seam inside the first frame"""
    ref = check(fr.make_case(P, rows=1, n_bits=40 * P + 11, P=P, phase0=P // 3, c=P - 9, skip=0, inverted=1, d=d, m=m, pad=True), off=1)
    assert len(ref[0][0]) == 41                              # the carry completes one more
    check(fr.make_case(P + 1, rows=3, n_bits=40 * P - 3, P=P, phase0=5, c=[0, 13, P - 1], inverted=2, d=d, m=m, pad=False, stride_extra=1,
                       frame_extra=1, carry_extra=1), off=0)


def test_aligned_layout_takes_the_dword_stores():
    for P, d in ((512, 0), (1024, 32), (192, 64)):
        for phase0 in (0, 3):
            check(fr.make_case(P + phase0, rows=64, n_bits=8 * P, P=P, phase0=phase0, c=[(7 * r) % P for r in range(64)], inverted=2, d=d, m=32,
                               pad=True), off=0)


def test_without_a_carry_pad_or_distances():
    import torch
    c = fr.make_case(5, rows=3, n_bits=700, P=67, phase0=11, c=[66, 1, 9], d=5, m=8, carry=False)
    check(c, off=1)
    check(c, off=1, errors=False)
    c = fr.make_case(6, rows=3, n_bits=700, P=67, phase0=11, c=[66, 1, 9], d=5, m=0)     # m = 0: the distances are not written
    out = Outputs(c)
    assert call(c, out) == _lib.OK
    assert (out.errors.cpu().numpy().view(np.uint32) == POISON * 0x01010101).all()
    torch.cuda.synchronize()


def test_wild_locks_and_carry_lengths_stay_inside_the_buffers():
    P = 67
    c = fr.make_case(7, rows=4, n_bits=500, P=P, phase0=3, c=[P, P + 1, 0xFFFFFFFF, 1 << 31], d=5, m=8, pad=True, stride_extra=1)
    c["lock"][:, 0] = (P, 0xFFFFFFFF, 1 << 31, 12345678)
    c["lock"][:, 1] = (0xFFFFFFFF, 2, 0, 1 << 31)
    ref = check(c, off=1)
    assert [rem for _, _, _, rem in ref] == [fr.cut(P, 3, int(ph), 0, 500)[2] for ph in c["lock"][:, 0]]


def test_rejections_launch_nothing():
    import torch
    code, pc, dec = decoder()
    c = fr.make_case(8, rows=2, n_bits=1000, P=64, phase0=0, c=5, d=8, m=8, marker=0x47, pad=True)
    out = Outputs(c)
    lib, h = _lib.load(), dec._handle._h
    d_bytes, d_carry = placed(c["bytes"], c["stride"], c["nb"], 0), placed(c["carry"], c["cstride"], c["cb"], 0)
    d_cbits = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_lock = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    d_pad = torch.zeros(7, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def extract(handle=h, bytes=d_bytes, stride=0, rows=2, n_bits=1000, P=64, phase0=0, lock=d_lock, carry=d_carry, cbits=d_cbits, cstride=0,
                marker=0x47, m=8, d=8, pad=d_pad, frames=out.frames, fstride=0, max_frames=16, n=out.n, errors=out.errors, carry_out=out.carry,
                cbits_out=out.carry_bits):
        return lib.vit_hip_frames_extract(handle, ptr(bytes), stride, rows, n_bits, P, phase0, ptr(lock), ptr(carry), ptr(cbits), cstride, marker,
                                          m, d, ptr(pad), ptr(frames), fstride, max_frames, ptr(n), ptr(errors), ptr(carry_out), ptr(cbits_out),
                                          stream)

    rejected = {
        "NULL handle": extract(handle=None), "NULL bytes": extract(bytes=None), "NULL lock": extract(lock=None),
        "NULL frames": extract(frames=None), "NULL n_frames": extract(n=None), "NULL carry_out": extract(carry_out=None),
        "NULL carry_bits_out": extract(cbits_out=None), "carry without its lengths": extract(cbits=None),
        "P = 7": extract(P=7, d=0, m=0, marker=0, max_frames=143), "P = 2^31": extract(P=1 << 31, max_frames=16), "phase0 = P": extract(phase0=64),
        "d = P": extract(d=64), "m = 65": extract(m=65), "m > P": extract(P=8, m=9, d=0, max_frames=125),
        "marker bits above m": extract(marker=0x147), "n_bits = 0": extract(n_bits=0), "n_bits = 2^32 - 64": extract(n_bits=(1 << 32) - 64, rows=1, P=1 << 30),
        "row stride below the row": extract(stride=124), "carry stride below the carry": extract(cstride=7),
        "frame stride below the frame": extract(fstride=6), "max_frames below the capacity": extract(max_frames=15),
        "2^31 rows": extract(rows=1 << 31),
    }
    torch.cuda.synchronize()
    for what, rc in rejected.items():
        assert rc == _lib.ERR_INVALID_ARG, (what, rc)
    assert (out.bytes == POISON).all().item() and (out.words.cpu().numpy().view(np.uint32) == POISON * 0x01010101).all()
    assert extract(rows=0) == _lib.OK                                       # no work
    torch.cuda.synchronize()
    assert (out.bytes == POISON).all().item() and (out.words.cpu().numpy().view(np.uint32) == POISON * 0x01010101).all()
    assert lib.vit_hip_frames_capacity(1000, 64) == 16 and lib.vit_hip_frames_capacity(1024, 64) == 16 and lib.vit_hip_frames_capacity(1025, 64) == 17
    assert lib.vit_hip_frames_capacity(1, 1 << 30) == 1 and lib.vit_hip_frames_capacity(5, 0) == 0
    # the bounds are tight, and a passing call does write
    assert extract(stride=125, cstride=8, fstride=7, max_frames=16) == _lib.OK
    torch.cuda.synchronize()
    assert out.n.cpu().numpy().tolist() == [15, 15] and out.carry_bits.cpu().numpy().tolist() == [40, 40]
    with pytest.raises(ValueError):
        dec.frames_extract(d_bytes.view(2, -1)[:, :125], 1000, 64, 0, d_lock, max_frames=3, out=None, drop_bits=64)
    with pytest.raises(_lib.VitHipError):
        dec.frames_extract(d_bytes[:250].view(2, 125), 1000, 64, 0, d_lock, marker=0x147, marker_bits=8)


def test_cut_invariance_over_five_calls_with_ping_ponged_carries():
    """one stream per row cut into 5 calls through the Python interface, one shorter than a period and one of a single bit: the frames in
    order, their distances and the last carry are those of ONE call"""
    import torch
    code, pc, dec = decoder()
    P, d, m, rows = 67, 5, 8, 3
    rng = np.random.default_rng(9)
    bits = rng.integers(0, 2, size=(rows, 10 * P + 13), dtype=np.uint8)
    pad = rng.integers(0, 256, size=(P - d + 7) // 8, dtype=np.uint8)
    lock = np.array([[20, 0, 0, 0], [66 + P, 1, 0, 0], [0, 1, 0, 0]], dtype=np.int32)
    d_lock, d_pad = torch.from_numpy(lock).cuda(), torch.from_numpy(pad).cuda()
    want = [frame_sync.frames_extract_numpy(np.packbits(bits[r]), bits.shape[1], P, 4, lock[r], None, 0, 0x47, m, d, pad) for r in range(rows)]
    got = [([], []) for _ in range(rows)]
    carry = carry_bits = None
    at = 0
    for n in (200, 1, 30, 300, bits.shape[1] - 531):
        d_bytes = torch.from_numpy(np.packbits(bits[:, at:at + n], axis=1)).cuda()
        frames, nf, errors, carry, carry_bits = dec.frames_extract(d_bytes, n, P, (4 + at) % P, d_lock, carry, carry_bits, 0x47, m, d, d_pad)
        nf = nf.cpu().numpy()
        for r in range(rows):
            got[r][0].extend(frames[r, :nf[r]].cpu().numpy())
            got[r][1].extend(errors[r, :nf[r]].cpu().numpy())
        at += n
    assert at == bits.shape[1]
    for r in range(rows):
        assert np.array_equal(np.array(got[r][0]), want[r][0]) and np.array_equal(np.array(got[r][1]), want[r][1]), r
        rem = int(carry_bits[r].item())
        assert rem == want[r][3] and np.array_equal(carry[r, :(rem + 7) // 8].cpu().numpy(), want[r][2])


def test_marker_search_then_frames_extract_captured_into_a_graph():
    """one chain, no parallel branch: the search writes the lock, the extraction reads it; replayed on two inputs"""
    import torch
    code, pc, dec = decoder()
    P, n_frames, d = 1024, 5, 32
    pad = frame_sync.ccsds_randomizer((P - d) // 8)
    streams = [fr.framed_stream(s, *CCSDS_ASM, P, n_frames, lead, pad) for s, lead in ((21, 100), (22, 900))]
    n_bits = min(b.size for b, _ in streams)
    rows = [np.packbits(b[:n_bits] ^ np.uint8(inv)) for (b, _), inv in zip(streams, (0, 1))]
    d_bytes = torch.from_numpy(rows[0]).cuda()
    d_pad = torch.from_numpy(pad).cuda()
    search_out = tuple(torch.empty(s, dtype=torch.int32, device="cuda") for s in ((1, P), (1, P), (1, 4)))
    cap = dec.frames_capacity(n_bits, P)
    out = (torch.empty((1, cap, (P - d) // 8), dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
           torch.empty((1, cap), dtype=torch.int32, device="cuda"), torch.empty((1, (P + 6) // 8), dtype=torch.uint8, device="cuda"),
           torch.empty(1, dtype=torch.int32, device="cuda"))

    def chain():
        dec.marker_search(d_bytes, n_bits, *CCSDS_ASM, P, out=search_out)
        dec.frames_extract(d_bytes, n_bits, P, 0, search_out[2], marker=CCSDS_ASM[0], marker_bits=32, drop_bits=d, pad=d_pad, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for row, (bits, payload), lead, inv in zip(rows, streams, (100, 900), (0, 1)):
        d_bytes.copy_(torch.from_numpy(row).cuda())
        for x in out:
            x.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        dd, cc = fr_search(row, n_bits, P)
        lock = frame_sync.marker_lock_numpy(dd, cc, 32)[0]
        assert tuple(lock[:2]) == (lead, inv)
        want = fr.extract_ints(row, n_bits, P, 0, int(lock[0]), int(lock[1]), None, 0, CCSDS_ASM[0], 32, d, pad)
        nf = int(out[1].item())
        assert nf == len(want[0]) == (n_bits - lead) // P
        assert np.array_equal(out[0][0, :nf].cpu().numpy(), want[0]) and np.array_equal(want[0], payload[:nf])
        assert out[2][0, :nf].cpu().numpy().tolist() == want[1] == [0] * nf
        assert (out[0][0, nf:] == POISON).all().item()
        assert int(out[4].item()) == want[3] and np.array_equal(out[3][0, :(want[3] + 7) // 8].cpu().numpy(), want[2])


def fr_search(row, n_bits, P):
    return frame_sync.marker_search_numpy(row, n_bits, *CCSDS_ASM, P)


# ---- the receivers ------------------------------------------------------------------------------------------------------------

WINDOW = 64


def coded(bits):
    """the noise-free symbols [steps][R] of a bit stream and its zero tail, from the device encoder"""
    import torch
    code, pc, dec = decoder()
    return dec.encode(torch.from_numpy(np.packbits(bits)[None]).cuda(), bits.size, tail=True)[0].cpu().numpy()


def ragged_pushes(rng, T):
    cuts = np.unique(rng.integers(1, T, size=9))
    return [(int(a), int(b)) for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [T]]))]


def emitted_per_call(rx, total):
    """the bits every internal call emitted: a segment emits its steps [0 or head, steps - tail or steps - (K-1))"""
    K = decoder()[0].K
    sizes = [steps - (K - 1 if end else rx.tail) - (0 if begin else rx.head) for steps, begin, end in rx.calls]
    assert sum(sizes) == total
    return sizes


def receiver_case(seed, inverted):
    P, d = RECEIVER["P"], RECEIVER["d"]
    pad = frame_sync.ccsds_randomizer((P - d) // 8)
    bits, payload = fr.framed_stream(seed, *CCSDS_ASM, P, RECEIVER["n_frames"], RECEIVER["lead"], pad, RECEIVER["trail"])
    sym = coded(bits)
    code, pc, dec = decoder()
    if inverted:
        sym = (pc.soft_decision_high + pc.soft_decision_low - sym.astype(np.int64)).astype(sym.dtype)
    return bits ^ np.uint8(inverted), payload, sym, pad


def check_taken(rx_calls_bits, bits, payload, pad, frames, errors, inverted):
    P, d = RECEIVER["P"], RECEIVER["d"]
    want_f, want_e, locks = fr.receiver_numpy(bits, rx_calls_bits, *CCSDS_ASM, P, d, pad)
    assert frames.dtype == np.uint8 and errors.dtype == np.int64 and frames.shape == (len(want_f), (P - d) // 8)
    assert np.array_equal(frames, want_f) and np.array_equal(errors, want_e)
    assert locks[FIRST_GOOD_FRAME] == (RECEIVER["lead"], inverted)
    assert len(frames) == RECEIVER["n_frames"] and np.array_equal(frames[FIRST_GOOD_FRAME:], payload[FIRST_GOOD_FRAME:])
    assert not errors[FIRST_GOOD_FRAME:].any()


def test_stream_decoder_takes_frames():
    import torch
    code, pc, dec = decoder()
    bits, payload, sym, pad = receiver_case(77, 0)
    d_sym = torch.from_numpy(sym).cuda()
    rx = StreamDecoder(dec, WINDOW, marker=CCSDS_ASM, period=RECEIVER["P"], frames=True, frame_drop_bits=RECEIVER["d"], frame_pad=pad)
    plain = StreamDecoder(dec, WINDOW)
    data, taken_f, taken_e = b"", [], []
    for a, b in ragged_pushes(np.random.default_rng(5), sym.shape[0]):
        data += rx.push(d_sym[a:b])
        plain.push(d_sym[a:b])
        f, e = rx.take_frames()
        taken_f.append(f)
        taken_e.append(e)
    data += rx.finish()
    plain.finish()
    f, e = rx.take_frames()
    assert rx.calls == plain.calls and len(rx.calls) > 3
    assert np.array_equal(np.unpackbits(np.frombuffer(data, dtype=np.uint8))[:bits.size], bits)
    again = rx.take_frames()
    assert again[0].shape == (0, (RECEIVER["P"] - RECEIVER["d"]) // 8) and again[1].size == 0
    check_taken(emitted_per_call(rx, rx.n_bits), np.unpackbits(np.frombuffer(data, dtype=np.uint8))[:rx.n_bits], payload, pad,
                np.concatenate(taken_f + [f]), np.concatenate(taken_e + [e]), 0)
    with pytest.raises(AttributeError):
        plain.take_frames()
    with pytest.raises(ValueError):
        StreamDecoder(dec, WINDOW, frames=True)
    with pytest.raises(ValueError):
        StreamDecoder(dec, WINDOW, marker=CCSDS_ASM, period=288, frames=True, frame_drop_bits=288)


def test_multi_stream_decoder_takes_the_frames_of_every_stream():
    import torch
    code, pc, dec = decoder()
    cases = [receiver_case(80 + i, int(i == 1)) for i in range(3)]
    d_sym = torch.from_numpy(np.stack([c[2] for c in cases])).cuda()
    pad = cases[0][3]
    rx = MultiStreamDecoder(dec, 3, WINDOW, marker=CCSDS_ASM, period=RECEIVER["P"], frames=True, frame_drop_bits=RECEIVER["d"],
                            frame_pad=torch.from_numpy(pad).cuda())
    data = [b""] * 3
    for a, b in ragged_pushes(np.random.default_rng(6), d_sym.shape[1]):
        data = [x + y for x, y in zip(data, rx.push(d_sym[:, a:b]))]
    data = [x + y for x, y in zip(data, rx.finish())]
    taken = rx.take_frames()
    assert len(taken) == 3 and len(rx.calls) > 3
    sizes = emitted_per_call(rx, rx.n_bits)
    for i, (bits, payload, _, _) in enumerate(cases):
        out_bits = np.unpackbits(np.frombuffer(data[i], dtype=np.uint8))[:rx.n_bits]
        # an inverted stream does not end in the zero tail the decoder assumes: its last bits, inside the trail, may differ
        assert out_bits.size == bits.size and np.array_equal(out_bits[:bits.size - RECEIVER["trail"]], bits[:bits.size - RECEIVER["trail"]])
        check_taken(sizes, out_bits, payload, pad, taken[i][0], taken[i][1], int(i == 1))
