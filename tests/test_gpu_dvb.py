"""BatchDecoder.deinterleave / dvb_derandomize (vit_hip_deinterleave_batch, vit_hip_dvb_derandomize_batch) on the GPU against the numpy
rules of viterbidecodercpp_amd.dvb (which tests/test_dvb_cpu.py holds against FIFOs and a shift register): every buffer whole, written or
not, from a 0xA5 fill -- five (branches, cell, packet) shapes, counts, fills, NULL history, strides with guard bytes at every dword
misalignment, counts and fills above their bounds, chunked calls against one; derandomising in place and out of place at every phase,
voted, without packets, with negative Reed-Solomon status, 204- and 188-byte packets; every rejected argument; the three calls in one
captured graph; and the whole DVB-S chain through StreamDecoder and MultiStreamDecoder, upright, inverted and across a re-lock."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, DVB_INTERLEAVER, DVB_RS_204_188, DVB_SYNC, BatchDecoder, MultiStreamDecoder, StreamDecoder, _lib,
                                   conv_deinterleave_numpy, conv_interleave_numpy, dvb, dvb_derandomize_numpy, dvb_randomize_numpy, frame_sync,
                                   rs_decode_numpy, rs_encode_numpy, synth)
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
SHAPES = [(12, 17, 204), (3, 2, 6), (5, 1, 10), (4, 3, 8), (3, 5, 9)]
IDS = ["-".join(map(str, s)) for s in SHAPES]
ROWS, MF = 3, 14


@functools.lru_cache(maxsize=None)
def decoder():
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    return code, pc, BatchDecoder(table, config)


def ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def poisoned(shape, lead=0):
    """a uint8 CUDA tensor of `shape` filled with 0xA5, `lead` bytes into its allocation"""
    import torch
    raw = torch.full((lead + int(np.prod(shape)),), POISON, dtype=torch.uint8, device="cuda")
    return raw[lead:].view(*shape)


def deint(B, M, n, x, counts, hist, fills, guard=0, lead=0, hguard=0):
    """one call on x [rows][mf][n] -> (out, n_out, hist_out, fill_out) as numpy buffer images, and the images the numpy rule predicts"""
    import torch
    dec = decoder()[2]
    rows, mf = x.shape[:2]
    H = dvb.history_packets(B, M, n)
    d_in = poisoned((rows, mf, n + guard), lead)
    d_in[..., :n] = torch.from_numpy(x).cuda()
    image_in = d_in.cpu().numpy()
    d_out = poisoned((rows, mf, n + guard), (lead + 1) % 4 if lead else 0)
    d_hist_out = poisoned((rows, H * n + hguard), lead)
    d_n_out = torch.full((rows,), POISON32, dtype=torch.int32, device="cuda")
    d_fill_out = torch.full((rows,), POISON32, dtype=torch.int32, device="cuda")
    d_n = None if counts is None else torch.tensor(counts, dtype=torch.int64).to(torch.int32).cuda()
    d_hist = d_fill = None
    if hist is not None:
        d_hist = poisoned((rows, H * n + hguard), (lead + 2) % 4 if lead else 0)
        d_hist[:, :H * n] = torch.from_numpy(hist.reshape(rows, H * n)).cuda()
        d_fill = torch.tensor(fills, dtype=torch.int64).to(torch.int32).cuda()
    got = dec.deinterleave(d_in[..., :n] if guard else d_in, d_n, B, M, d_hist[:, :H * n] if hguard and hist is not None else d_hist, d_fill,
                           out=(d_out[..., :n] if guard else d_out, d_n_out, d_hist_out[:, :H * n] if hguard else d_hist_out, d_fill_out))
    torch.cuda.synchronize()
    assert got[1] is d_n_out and np.array_equal(d_in.cpu().numpy(), image_in)            # the input is only read
    want_out = np.full((rows, mf, n + guard), POISON, dtype=np.uint8)
    want_hist = np.full((rows, H * n + hguard), POISON, dtype=np.uint8)
    want_n, want_fill = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        nf = mf if counts is None else min(counts[r], mf)
        out, nout, new, keep = conv_deinterleave_numpy(x[r], B, M, None if hist is None else hist[r], 0 if hist is None else fills[r], nf)
        want_out[r, :nout, :n] = out
        want_hist[r, (H - keep) * n:H * n] = new[H - keep:].reshape(-1)
        want_n[r], want_fill[r] = nout, keep
    have = (d_out.cpu().numpy(), d_n_out.cpu().numpy().astype(np.int64), d_hist_out.cpu().numpy(), d_fill_out.cpu().numpy().astype(np.int64))
    return have, (want_out, want_n, want_hist, want_fill)


def same(have, want, where=None):
    for k, (a, b) in enumerate(zip(have, want)):
        assert np.array_equal(a, b), (where, k, np.argwhere(a != b)[:6].tolist())


@pytest.mark.parametrize("B,M,n", SHAPES, ids=IDS)
def test_counts_fills_null_history_and_guard_bytes(B, M, n):
    H = dvb.history_packets(B, M, n)
    rng = np.random.default_rng(n)
    x = rng.integers(0, 256, size=(ROWS, MF, n), dtype=np.uint8)
    hist = rng.integers(0, 256, size=(ROWS, H, n), dtype=np.uint8)
    counts, fills = [0, 5, 14], [0, H, min(4, H)]
    for guard, lead in ((0, 0), (1, 1), (3, 2), (1, 3)):
        same(*deint(B, M, n, x, counts, hist, fills, guard, lead, hguard=guard), where=("hist", guard, lead))
        same(*deint(B, M, n, x, counts, None, None, guard, lead), where=("null", guard, lead))
    same(*deint(B, M, n, x, None, hist, [H, 1, 0]), where="all frames")
    same(*deint(B, M, n, x, [5, 14, 0], hist, [0, H, min(4, H)]), where="rotated")
    # a count above max_frames reads as max_frames, a fill above H as H; neither takes the kernel out of its buffers
    same(*deint(B, M, n, x, [MF + 1, 0xFFFFFFFF, 3], hist, [H + 1, 0xFFFFFFFF, 0x80000000], 3, 1, hguard=2), where="above")


@pytest.mark.parametrize("B,M,n", SHAPES, ids=IDS)
def test_five_calls_give_what_one_gives(B, M, n):
    import torch
    dec = decoder()[2]
    x = np.random.default_rng(5).integers(0, 256, size=(2, 40, n), dtype=np.uint8)
    one = [conv_deinterleave_numpy(x[r], B, M) for r in range(2)]
    hist = fill = None
    outs, at = [[], []], 0
    for size in (1, 0, 10, 12, 17):
        d_in = torch.from_numpy(np.ascontiguousarray(x[:, at:at + 17])).cuda()            # room for 17; the count says how many
        if d_in.shape[1] < 17:
            d_in = torch.cat([d_in, torch.zeros((2, 17 - d_in.shape[1], n), dtype=torch.uint8, device="cuda")], dim=1)
        d_n = torch.full((2,), size, dtype=torch.int32, device="cuda")
        out, n_out, hist, fill = dec.deinterleave(d_in, d_n, B, M, hist, fill)
        torch.cuda.synchronize()
        for r in range(2):
            outs[r].append(out[r, :int(n_out[r])].cpu().numpy())
        at += size
    H = dvb.history_packets(B, M, n)
    for r in range(2):
        assert np.array_equal(np.concatenate(outs[r]), one[r][0])
        assert int(fill[r]) == one[r][3] == H and np.array_equal(hist[r].cpu().numpy().reshape(H, n), one[r][2])


def test_more_packets_than_one_block_takes():
    """DVB-S's shape at 200 packets a row: four output blocks a row, the last one ragged, beside the history block"""
    B, M, n = 12, 17, 204
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, size=(2, 200, n), dtype=np.uint8)
    hist = rng.integers(0, 256, size=(2, 11, n), dtype=np.uint8)
    same(*deint(B, M, n, x, [200, 139], hist, [11, 3], 1, 3, hguard=1))


def derand(x, counts, phases, status, in_place, guard=0, lead=0):
    """one call on x [rows][mf][nb] -> images of (out, phase_out, sync_errors) and what the numpy rule predicts"""
    import torch
    dec = decoder()[2]
    rows, mf, nb = x.shape
    d_in = poisoned((rows, mf, nb + guard), lead)
    d_in[..., :nb] = torch.from_numpy(x).cuda()
    image_in = d_in.cpu().numpy()
    width = nb if in_place else 188
    d_out = None if in_place else poisoned((rows, mf, 188 + guard), (lead + 1) % 4 if lead else 0)
    d_n = None if counts is None else torch.tensor(counts, dtype=torch.int64).to(torch.int32).cuda()
    d_phase = None if phases is None else torch.tensor(phases, dtype=torch.int64).to(torch.int32).cuda()
    d_status = None if status is None else torch.from_numpy(status.astype(np.int32)).cuda()
    d_phase_out = torch.full((rows,), POISON32, dtype=torch.int32, device="cuda")
    d_errors = torch.full((rows, mf), POISON32, dtype=torch.int32, device="cuda")
    view = d_in[..., :nb] if guard else d_in
    dec.dvb_derandomize(view, d_n, d_phase, d_status, out=None if in_place else (d_out[..., :188] if guard else d_out), phase_out=d_phase_out,
                        sync_errors=d_errors, in_place=in_place)
    torch.cuda.synchronize()
    want_out = image_in.copy() if in_place else np.full((rows, mf, width + guard), POISON, dtype=np.uint8)
    want_phase = np.zeros(rows, dtype=np.int64)
    want_errors = np.full((rows, mf), POISON32, dtype=np.int64)
    for r in range(rows):
        nf = mf if counts is None else min(counts[r], mf)
        out, errors, nxt = dvb_derandomize_numpy(x[r], None if phases is None else phases[r], None if status is None else status[r], nf)
        want_out[r, :len(out), :188] = out
        want_errors[r, :len(errors)] = errors
        want_phase[r] = nxt
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy(), image_in)
    have = ((d_in if in_place else d_out).cpu().numpy(), d_phase_out.cpu().numpy().view(np.uint32).astype(np.int64), d_errors.cpu().numpy().astype(np.int64))
    return have, (want_out, want_phase, want_errors)


def scrambled_rows(seed, rows, mf, nb, phases, flips=0):
    """rows of randomised packets whose packet 0 is packet phases[r] of its group, `flips` sync bytes per row with a wrong bit"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(rows, mf, nb), dtype=np.uint8)
    for r in range(rows):
        ts = rng.integers(0, 256, size=(mf, 188), dtype=np.uint8)
        ts[:, 0] = 0x47
        x[r, :, :188] = dvb_randomize_numpy(ts, phases[r])
        for f in rng.choice(mf, size=flips, replace=False):
            x[r, f, 0] ^= 1 << int(rng.integers(0, 8))
    return x


@pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("nb", [204, 188])
def test_every_phase_known_and_voted(nb, in_place):
    status = np.where(np.random.default_rng(4).integers(0, 3, size=(4, MF)) == 0, -1, 2)
    assert (status < 0).any()
    for first in (0, 4):
        phases = [first, first + 1, first + 2, first + 3]
        x = scrambled_rows(first, 4, MF, nb, phases, flips=2)
        for guard, lead in ((0, 0), (1, 1), (3, 2), (1, 3)):
            same(*derand(x, None, phases, status, in_place, guard, lead), where=("known", guard, lead))
        same(*derand(x, None, None, None, in_place, 1, 1), where="all voted")
        same(*derand(x, [14, 9, 0, 1], [8, -1, 0xFFFFFFFF, 77], status, in_place, 3, 3), where="voted per row")
        same(*derand(x, [0, 3, MF + 5, 0], [8, phases[1], phases[2], 5], None, in_place), where="no packets")
        # a phase that is not the transmitter's is taken at its word
        same(*derand(x, None, [(p + 3) % 8 for p in phases], status, in_place), where="wrong")
    have, want = derand(scrambled_rows(9, 2, MF, nb, [6, 1]), [0, 0], None, None, in_place)
    same(have, want)
    assert have[1].tolist() == [0xFFFFFFFF] * 2


def test_many_packets_a_row_vote_in_every_block():
    """out of place a long row is cut into blocks of 32 packets that each vote over all of it; in place it is one block"""
    x = scrambled_rows(21, 2, 150, 204, [5, 2], flips=9)
    for in_place in (False, True):
        same(*derand(x, [150, 97], None, None, in_place, 1, 1), where=in_place)
        same(*derand(x, [150, 97], [5, 8], None, in_place), where=in_place)


def test_rejections_launch_nothing():
    import torch
    L, dec = _lib.load(), decoder()[2]
    h = dec._handle._h
    B, M, n, rows, mf = 12, 17, 204, 2, 3
    H = 11
    buf = torch.full((8 * rows * mf * n + 4 * rows * H * n,), POISON, dtype=torch.uint8, device="cuda")
    cnt = torch.full((8 * rows,), POISON32, dtype=torch.int32, device="cuda")
    a = buf.data_ptr()
    b, hi, ho = a + rows * mf * n, a + 2 * rows * mf * n, a + 2 * rows * mf * n + rows * H * n
    c = cnt.data_ptr()
    nfr, fin, nout, fout = c, c + 4 * rows, c + 8 * rows, c + 12 * rows
    good = dict(h=h, src=a, stride=0, rows=rows, mf=mf, nfr=nfr, B=B, M=M, n=n, hi=hi, fin=fin, hs=0, dst=b, os=0, nout=nout, ho=ho, fout=fout)

    def call(**kw):
        k = {**good, **kw}
        return L.vit_hip_deinterleave_batch(k["h"], k["src"], k["stride"], k["rows"], k["mf"], k["nfr"], k["B"], k["M"], k["n"], k["hi"], k["fin"],
                                            k["hs"], k["dst"], k["os"], k["nout"], k["ho"], k["fout"], None)

    bad = [dict(h=None), dict(src=None), dict(dst=None), dict(nout=None), dict(ho=None), dict(fout=None), dict(fin=None), dict(B=1), dict(M=0),
           dict(n=200), dict(n=0), dict(M=2000), dict(B=2, M=8193, n=16384), dict(stride=203), dict(os=203), dict(hs=H * n - 1),
           dict(dst=a), dict(dst=a + rows * mf * n - 1), dict(dst=hi + 5), dict(dst=ho), dict(ho=hi), dict(ho=a + 7), dict(ho=hi + H * n),
           dict(nout=nfr), dict(fout=fin), dict(nout=fin), dict(fout=nfr), dict(fout=nout), dict(rows=1 << 31), dict(mf=1 << 31)]
    for kw in bad:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert b"overlap" in L.vit_hip_last_error() or b"2^31" in L.vit_hip_last_error()
    assert call(rows=0) == _lib.OK and call(mf=0) == _lib.OK and call(rows=0, B=1) == _lib.ERR_INVALID_ARG
    assert call(hi=None, fin=None) == _lib.OK                                             # no history: the fill is not asked for
    torch.cuda.synchronize()
    assert (buf[rows * mf * n:2 * rows * mf * n] == POISON).all().item()                  # rows of 0xA5 without history give no output
    buf.fill_(POISON)
    cnt.fill_(POISON32)

    pin, pout = c, c + 4 * rows
    goodr = dict(h=h, src=a, stride=0, n=204, rows=rows, mf=mf, nfr=None, pin=pin, st=None, dst=b, os=0, pout=pout, se=None)

    def callr(**kw):
        k = {**goodr, **kw}
        return L.vit_hip_dvb_derandomize_batch(k["h"], k["src"], k["stride"], k["n"], k["rows"], k["mf"], k["nfr"], k["pin"], k["st"], k["dst"],
                                               k["os"], k["pout"], k["se"], None)

    badr = [dict(h=None), dict(src=None), dict(dst=None), dict(pout=None), dict(n=187), dict(stride=203), dict(os=187), dict(dst=a + 1),
            dict(dst=a, os=188), dict(dst=a + (rows * mf - 1) * 204 + 187), dict(src=a + 300, dst=a, os=204), dict(pout=pin), dict(rows=1 << 31),
            dict(mf=1 << 31)]
    for kw in badr:
        assert callr(**kw) == _lib.ERR_INVALID_ARG, kw
    assert callr(rows=0) == _lib.OK and callr(mf=0) == _lib.OK and callr(rows=0, n=100) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (buf == POISON).all().item() and (cnt == POISON32).all().item()
    with pytest.raises(ValueError):
        dec.deinterleave(buf[:6 * 200].view(2, 3, 200), None, 12, 17)
    with pytest.raises(ValueError):
        dec.dvb_derandomize(buf[:6 * 100].view(2, 3, 100))


def dvb_transmit(rng, n_packets):
    """(transport packets [N][188] with their sync byte, the interleaved 204-byte packets a transmitter sends)"""
    ts = rng.integers(0, 256, size=(n_packets, 188), dtype=np.uint8)
    ts[:, 0] = 0x47
    sent = conv_interleave_numpy(rs_encode_numpy(DVB_RS_204_188, dvb_randomize_numpy(ts), 1), *DVB_INTERLEAVER)
    return ts, sent


def test_deinterleave_rs_decode_and_derandomize_in_one_graph():
    import torch
    dec = decoder()[2]
    B, M = DVB_INTERLEAVER
    n, H, mf, rows = 204, 11, 30, 2
    rng = np.random.default_rng(31)
    cases = []
    for _ in range(2):
        ts = rng.integers(0, 256, size=(rows, mf, 188), dtype=np.uint8)
        ts[..., 0] = 0x47
        words = np.array([rs_encode_numpy(DVB_RS_204_188, dvb_randomize_numpy(ts[r]), 1) for r in range(rows)])
        for r in range(rows):
            for f in range(mf):
                for at in rng.choice(n, size=(f + r) % 11, replace=False):                # up to 10 byte errors a codeword: beyond t = 8 too
                    words[r, f, at] ^= int(rng.integers(1, 256))
        cases.append((ts, np.array([conv_interleave_numpy(words[r], B, M) for r in range(rows)])))
    d_in = torch.empty((rows, mf, n), dtype=torch.uint8, device="cuda")
    d_n = torch.tensor([mf, mf - 4], dtype=torch.int32, device="cuda")
    hist = (torch.zeros((rows, H * n), dtype=torch.uint8, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda"))
    outs = (torch.empty((rows, mf, n), dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda"),
            torch.empty((rows, H * n), dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda"))
    status = torch.empty((rows, mf, 1), dtype=torch.int32, device="cuda")
    packets = torch.empty((rows, mf, 188), dtype=torch.uint8, device="cuda")
    phase_out = torch.empty(rows, dtype=torch.int32, device="cuda")
    errors = torch.empty((rows, mf), dtype=torch.int32, device="cuda")

    def chain():
        dec.deinterleave(d_in, d_n, B, M, hist[0], hist[1], out=outs)
        dec.rs_decode(DVB_RS_204_188, outs[0], outs[1], 1, status=status)
        dec.dvb_derandomize(outs[0], outs[1], None, status, out=packets, phase_out=phase_out, sync_errors=errors)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for ts, x in cases:
        d_in.copy_(torch.from_numpy(x).cuda())
        for buf in (outs[0], packets):
            buf.fill_(POISON)
        status.fill_(POISON32)
        errors.fill_(POISON32)
        graph.replay()
        torch.cuda.synchronize()
        for r, nf in enumerate((mf, mf - 4)):
            out, nout, _, keep = conv_deinterleave_numpy(x[r], B, M, None, 0, nf)
            fixed, st = rs_decode_numpy(DVB_RS_204_188, out, 1)
            want, want_errors, nxt = dvb_derandomize_numpy(fixed, None, st[:, 0])
            assert int(outs[1][r]) == nout == nf - H and int(outs[3][r]) == keep == H and int(phase_out[r]) == nxt
            assert np.array_equal(status[r, :nout, 0].cpu().numpy(), st[:, 0]) and (st == -1).any() and (st > 0).any()
            assert np.array_equal(packets[r, :nout].cpu().numpy(), want) and np.array_equal(errors[r, :nout].cpu().numpy(), want_errors)
            good = st[:, 0] >= 0
            assert good.sum() >= 5 and np.array_equal(want[good], ts[r][:nout][good])
            assert (packets[r, nout:] == POISON).all().item() and (status[r, nout:] == POISON32).all().item()


# ---- the whole chain ---------------------------------------------------------------------------------------------------------------

CHAIN_DB = 3.0


def chain_symbols(seed, n_packets, lead, inverted=False, drop=None):
    """transport packets -> energy dispersal -> RS(204,188) -> interleaver -> `lead` random bits in front -> (complemented) -> (bits
    dropped at `drop` = (position, count)) -> the package's K = 7 R = 1/2 encoder -> noise.  returns (ts [N][188], symbols [steps][R])"""
    import torch
    conv, pc, dec = decoder()
    rng = np.random.default_rng(seed)
    ts, sent = dvb_transmit(rng, n_packets)
    bits = np.concatenate([rng.integers(0, 2, size=lead, dtype=np.uint8), np.unpackbits(sent.reshape(-1))])
    if inverted:
        bits = bits ^ 1
    if drop is not None:
        bits = np.concatenate([bits[:drop[0]], bits[drop[0] + drop[1]:]])
    bits = bits[:bits.size - bits.size % 8]
    sym = dec.encode(torch.from_numpy(np.packbits(bits)).cuda()[None], bits.size, tail=True).cpu().numpy()[0]
    mid = (pc.soft_decision_high + pc.soft_decision_low) / 2
    noisy = synth.quantise_numpy((sym > mid).astype(np.uint8), pc.soft_decision_high, pc.soft_decision_low, CHAIN_DB, conv.R, rng, pc.soft_dtype)
    return ts, noisy


def emitted_per_call(rx):
    K = decoder()[0].K
    sizes = [steps - (K - 1 if end else rx.tail) - (0 if begin else rx.head) for steps, begin, end in rx.calls]
    assert sum(sizes) == rx.n_bits
    return sizes


def chain_numpy(bits, chunks):
    """what a receiver with marker=DVB_SYNC, period=1632, frames, rs, deinterleave and dvb_derandomize does, by the numpy rules alone, over
    the calls that emit `chunks` bits each.  returns (packets [k][188], sync_errors [k], rs_status [k][1], re-locks seen)"""
    value, m = DVB_SYNC
    P, (B, M) = 1632, DVB_INTERLEAVER
    distance, count = np.zeros((1, P), dtype=np.int64), np.zeros((1, P), dtype=np.int64)
    lock, before = np.zeros(4, dtype=np.int64), (0, 0)
    carry, cbits, at = None, 0, 0
    hist, fill, phase, relocks = None, 0, None, 0
    packets, errors, status = [], [], []
    for n in chunks:
        seg = bits[at:at + n]
        hb = min(m - 1, at)
        if n + hb >= m:
            word = int("".join(map(str, bits[at - hb:at])), 2) if hb else 0
            dd, cc = frame_sync.marker_search_numpy(np.packbits(seg), n, value, m, P, at % P, [word], hb)
            distance, count = distance + dd, count + cc
            lock = frame_sync.marker_lock_numpy(distance, count, m)[0]
        if n:
            fr, _, carry, cbits = frame_sync.frames_extract_numpy(np.packbits(seg), n, P, at % P, lock, carry, cbits, value, m)
            if (int(lock[0]), int(lock[1])) != before:
                fill, phase, relocks = 0, None, relocks + 1
            before = (int(lock[0]), int(lock[1]))
            out, nout, hist, fill = conv_deinterleave_numpy(fr.reshape(-1, 204), B, M, hist, fill)
            fixed, st = rs_decode_numpy(DVB_RS_204_188, out, 1) if nout else (out, np.zeros((0, 1), dtype=np.int32))
            ts, er, nxt = dvb_derandomize_numpy(fixed, phase, st[:, 0])
            phase = None if nxt > 7 else nxt
            packets += list(ts)
            errors += list(er)
            status += list(st)
        at += n
    return (np.array(packets, dtype=np.uint8).reshape(-1, 188), np.array(errors, dtype=np.int64), np.array(status, dtype=np.int32).reshape(-1, 1),
            relocks)


def receive(rx, d_sym, cuts, multi=False):
    """push the symbols cut at `cuts` (steps), finish with the rest; what take_frames() gave after every call, and the decoded bits"""
    R = decoder()[0].R
    taken, data = [], None
    edges = [0] + list(cuts) + [d_sym.shape[-2]]
    for a, b in zip(edges[:-1], edges[1:]):
        part = d_sym[..., a:b, :]
        got = rx.finish(part) if b == edges[-1] else rx.push(part)
        data = got if data is None else ([x + y for x, y in zip(data, got)] if multi else data + got)
        taken.append(rx.take_frames())
    return taken, data


def joined(taken):
    return tuple(np.concatenate([t3[k] for t3 in taken]) for k in range(3))


def check_against_the_rules(rx, taken, data, ts):
    packets, errors, status = joined(taken)
    decoded = np.unpackbits(np.frombuffer(data, dtype=np.uint8))[:rx.n_bits]
    cpu_packets, cpu_errors, cpu_status, relocks = chain_numpy(decoded, emitted_per_call(rx))
    assert packets.shape == cpu_packets.shape and packets.shape[1] == 188 and status.dtype == np.int32 and status.shape == (len(packets), 1)
    assert np.array_equal(packets, cpu_packets) and np.array_equal(errors, cpu_errors) and np.array_equal(status, cpu_status)
    where = {row.tobytes(): k for k, row in enumerate(ts)}
    good = status[:, 0] >= 0
    index = [where.get(row.tobytes(), -1) for row in packets[good]]
    assert min(index) >= 0                                                             # every packet the outer code vouches for was sent
    print("packets", len(packets), "good", int(good.sum()), "corrected bytes", int(status[good].sum()), "sync errors", int(errors.sum()))
    return cpu_packets, cpu_status, index, relocks


@pytest.mark.parametrize("inverted", [False, True], ids=["upright", "inverted"])
def test_the_whole_dvb_chain_through_the_stream_decoder(inverted):
    import torch
    conv, pc, dec = decoder()
    N, H = 60, 11
    ts, noisy = chain_symbols(41, N, 776, inverted)
    d_sym = torch.from_numpy(noisy).cuda()
    rx = StreamDecoder(dec, 1024, marker=DVB_SYNC, period=1632, frames=True, rs=DVB_RS_204_188, deinterleave=DVB_INTERLEAVER, dvb_derandomize=True)
    assert [x.shape for x in rx.take_frames()] == [(0, 188), (0,), (0, 1)]
    taken, data = receive(rx, d_sym, [30 * 1632 + 5, 30 * 1632 + 1500, 41 * 1632 + 333, 52 * 1632])
    assert sum(len(t3[0]) > 0 for t3 in taken) >= 3                                    # the packets came out over several takes
    cpu_packets, cpu_status, index, relocks = check_against_the_rules(rx, taken, data, ts)
    assert relocks == 1                                                                # the lock the first call found holds
    # the numpy rules alone recover every packet past the H that fill the delay lines: the count is theirs, exactly
    assert (cpu_status >= 0).all() and len(cpu_packets) == N - H and np.array_equal(cpu_packets, ts[:N - H])
    assert index == list(range(N - H)) and rx.marker_lock[1] == int(inverted)


def test_two_streams_through_the_multi_stream_decoder():
    import torch
    conv, pc, dec = decoder()
    N, H = 50, 11
    both = [chain_symbols(seed, N, 776) for seed in (43, 44)]
    d_sym = torch.from_numpy(np.stack([b[1] for b in both])).cuda()
    rx = MultiStreamDecoder(dec, 2, 1024, marker=DVB_SYNC, period=1632, frames=True, rs=DVB_RS_204_188, deinterleave=DVB_INTERLEAVER,
                            dvb_derandomize=True)
    taken, data = receive(rx, d_sym, [30 * 1632 + 64, 31 * 1632, 44 * 1632 + 901], multi=True)
    sizes = emitted_per_call(rx)
    for i in range(2):
        packets, errors, status = joined([t[i] for t in taken])
        decoded = np.unpackbits(np.frombuffer(data[i], dtype=np.uint8))[:rx.n_bits]
        cpu_packets, cpu_errors, cpu_status, relocks = chain_numpy(decoded, sizes)
        assert np.array_equal(packets, cpu_packets) and np.array_equal(errors, cpu_errors) and np.array_equal(status, cpu_status)
        assert relocks == 1 and (cpu_status >= 0).all() and len(cpu_packets) == N - H and np.array_equal(packets, both[i][0][:N - H])


def test_a_relock_restarts_fill_and_group_phase():
    """13 bits vanish inside packet 32 of 200.  The first call (30 packets) locks and delivers packets 0 ..; the totals of the second (up
    to packet 130) name the new phase, so that call's extraction cuts there: on the device the fill goes back to 0 and the group phase
    to unknown, the delay lines fill afresh with H packets and the phase is voted anew (the packets behind the slip descramble only at
    their own place in a group of eight), and every later packet comes out."""
    import torch
    conv, pc, dec = decoder()
    N, H, slip = 200, 11, 32
    ts, noisy = chain_symbols(47, N, 400, drop=(400 + slip * 1632 + 700, 13))
    d_sym = torch.from_numpy(noisy).cuda()
    rx = StreamDecoder(dec, 1024, marker=DVB_SYNC, period=1632, frames=True, rs=DVB_RS_204_188, deinterleave=DVB_INTERLEAVER, dvb_derandomize=True)
    taken, data = receive(rx, d_sym, [30 * 1632 + 9, 130 * 1632 + 77, 170 * 1632 + 5])
    cpu_packets, cpu_status, index, relocks = check_against_the_rules(rx, taken, data, ts)
    assert relocks == 2
    first, second = [k for k in index if k < slip], [k for k in index if k > slip]
    assert first == list(range(len(first))) and len(first) >= 10
    # the stream ends 16 bits short of its last packet (13 dropped, 3 cut to whole bytes): the last input is packet N - 2
    assert second == list(range(second[0], N - 1 - H)) and slip < second[0] <= slip + 3


def test_the_keywords_are_checked_and_change_nothing_when_absent():
    conv, pc, dec = decoder()
    kw = dict(marker=DVB_SYNC, period=1632, frames=True)
    for bad in (dict(frames=False), dict(frame_drop_bits=8), dict(frame_pad=np.zeros(204, dtype=np.uint8)), dict(period=1640),
                dict(rs=DVB_RS_204_188, rs_interleave=2), dict(deinterleave=(1, 17)), dict(deinterleave=(12, 0)), dict(deinterleave=(12, 3000))):
        with pytest.raises(ValueError):
            StreamDecoder(dec, 1024, **{**kw, "deinterleave": DVB_INTERLEAVER, **bad})
    with pytest.raises(ValueError):
        StreamDecoder(dec, 1024, **kw, dvb_derandomize=True)
    with pytest.raises(ValueError):
        StreamDecoder(dec, 1024, marker=DVB_SYNC, period=96, frames=True, deinterleave=(3, 2), dvb_derandomize=True)
    plain = StreamDecoder(dec, 1024, **kw)
    assert plain._chain.branches is None and [x.shape for x in plain.take_frames()] == [(0, 204), (0,)]
