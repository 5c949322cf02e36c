"""The argument rules of the Python host layer, one case per rule: every `raise ValueError` of BatchDecoder's six outer-chain methods
(marker_search, frames_extract, rs_decode, deinterleave, dvb_derandomize and the packet / count rules under them) and of encode,
channel_errors, update_resume, decode_stream, decode_streams, decode_tail_biting, sync_build and depuncture is reached by a case of
CASES, listed beside the rule it hits.  A case starts from a call that is accepted, spoils one argument and must be rejected on the
host, before any launch: every tensor of the call, the outputs prefilled with 0xA5 among them, holds afterwards what it held before.
The test_edge_* tests are the layouts the rules tolerate on purpose; each must be accepted and give what the plain layout gives (an
empty tensor gets past the host rules in any layout; what the C ABI then says to its NULL address is the same for all)."""
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import CCSDS_RS_255_223, COMMON_CODES, DVB_RS_204_188, BatchDecoder, _lib
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

ROWS, N_BITS, PERIOD, MARKER, MARKER_BITS = 2, 100, 16, 0x47, 8
NB, CAP, QB, CB = 13, 7, 2, 2                   # ceil(100/8) bytes, ceil(100/16) frames, ceil(16/8) frame bytes, ceil(15/8) carry bytes
MF, PACKET, B, M, H = 3, 204, 12, 17, 11        # packets [2][3][204]; H = ceil(11 * 17 * 12 / 204) history packets
L, WINDOW, HEAD, TAIL = 64, 64, 48, 48
T, PITCH, EMITTED = HEAD + WINDOW + TAIL, 3 * WINDOW, (HEAD + WINDOW + 7) // 8      # a BEGIN segment emits its steps [0, T - tail)


@functools.lru_cache(maxsize=None)
def decoder():
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    return BatchDecoder(table, config)


def torch_():
    import torch
    return torch


def poisoned(shape, dtype):
    """a CUDA tensor of `shape` whose every byte is 0xA5"""
    t = torch_()
    n = int(np.prod(shape)) * t.empty(0, dtype=dtype).element_size()
    return t.full((n,), 0xA5, dtype=t.uint8, device="cuda").view(dtype).view(*shape)


def rand_u8(shape, seed=1):
    return torch_().from_numpy(np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)).cuda()


def rand_sym(shape, seed=2):
    return torch_().from_numpy(np.random.default_rng(seed).integers(-100, 100, size=shape).astype(np.int16)).cuda()


def zeros32(*shape):
    t = torch_()
    return t.zeros(shape, dtype=t.int32, device="cuda")


# ---- one accepted call per method: (bound method, its arguments by name) ----

def base_marker_search():
    t = torch_()
    return decoder().marker_search, dict(bytes=rand_u8((ROWS, NB)), n_bits=N_BITS, marker=MARKER, marker_bits=MARKER_BITS, period=PERIOD,
                                         out=(poisoned((ROWS, PERIOD), t.int32), poisoned((ROWS, PERIOD), t.int32), poisoned((ROWS, 4), t.int32)))


def base_frames_extract():
    t = torch_()
    out = (poisoned((ROWS, CAP, QB), t.uint8), poisoned((ROWS,), t.int32), poisoned((ROWS, CAP), t.int32), poisoned((ROWS, CB), t.uint8),
           poisoned((ROWS,), t.int32))
    return decoder().frames_extract, dict(bytes=rand_u8((ROWS, NB)), n_bits=N_BITS, period=PERIOD, phase0=0, lock=zeros32(ROWS, 4),
                                          carry=rand_u8((ROWS, CB)), carry_bits=zeros32(ROWS), marker=MARKER, marker_bits=MARKER_BITS,
                                          pad=rand_u8((QB,)), out=out)


def base_rs_decode(code=DVB_RS_204_188, interleave=1):
    t = torch_()
    n = code.n * interleave
    return decoder().rs_decode, dict(code=code, frames=rand_u8((ROWS, MF, n)), n_frames=zeros32(ROWS) + MF, interleave=interleave,
                                     out=poisoned((ROWS, MF, n), t.uint8), status=poisoned((ROWS, MF, interleave), t.int32))


def base_rs_decode_ccsds():
    return base_rs_decode(CCSDS_RS_255_223, 2)


def base_deinterleave():
    t = torch_()
    out = (poisoned((ROWS, MF, PACKET), t.uint8), poisoned((ROWS,), t.int32), poisoned((ROWS, H * PACKET), t.uint8), poisoned((ROWS,), t.int32))
    return decoder().deinterleave, dict(packets=rand_u8((ROWS, MF, PACKET)), n_frames=zeros32(ROWS) + MF, branches=B, cell=M,
                                        hist=rand_u8((ROWS, H * PACKET)), fill=zeros32(ROWS) + H, out=out)


def base_dvb_derandomize():
    t = torch_()
    return decoder().dvb_derandomize, dict(packets=rand_u8((ROWS, MF, PACKET)), n_frames=zeros32(ROWS) + MF, phase=zeros32(ROWS),
                                           rs_status=zeros32(ROWS, MF, 1), out=poisoned((ROWS, MF, 188), t.uint8),
                                           phase_out=poisoned((ROWS,), t.int32), sync_errors=poisoned((ROWS, MF), t.int32))


def base_encode():
    t = torch_()
    return decoder().encode, dict(bytes=rand_u8((ROWS, L // 8)), L=L, out=poisoned((ROWS, L + 6, 2), t.int16),
                                  end_state_out=poisoned((ROWS,), t.int32))


def base_channel_errors():
    return decoder().channel_errors, dict(symbols=rand_sym((ROWS, L + 6, 2)), bytes=rand_u8((ROWS, L // 8)), L=L)


def base_update_resume():
    t = torch_()
    return decoder().update_resume, dict(symbols=rand_sym((ROWS, L + 6, 2)), L=L, first_step=0, metrics=decoder().reset_batch(ROWS),
                                         renorm_out=poisoned((ROWS,), t.int64))


def base_decode_stream():
    t = torch_()
    return decoder().decode_stream, dict(symbols=rand_sym((T, 2)), window=WINDOW, out=poisoned((EMITTED,), t.uint8))


def base_decode_streams():
    t = torch_()
    return decoder().decode_streams, dict(symbols=rand_sym((ROWS, PITCH, 2)), steps=T, window=WINDOW, out=poisoned((ROWS, EMITTED), t.uint8))


def base_decode_tail_biting():
    t = torch_()
    return decoder().decode_tail_biting, dict(symbols=rand_sym((ROWS, L, 2)), L=L, out=poisoned((ROWS, L // 8), t.uint8),
                                              end_state_out=poisoned((ROWS,), t.int32), ok_out=poisoned((ROWS,), t.uint8))


def base_sync_build():
    t = torch_()
    return decoder().sync_build, dict(received=rand_sym((400,)), hypotheses=[(0, 0), (1, 0)], steps=L, out=poisoned((2, L, 2), t.int16))


MASK = np.array([1, 1, 1, 0] * 8)                # rate 2/3 over 16 steps: 24 of 32 symbols are sent


def base_depuncture():
    t = torch_()
    return decoder().depuncture, dict(punctured=rand_sym((ROWS, 24)), mask=MASK, out=poisoned((ROWS, 16, 2), t.int16))


# ---- how a case spoils an argument ----

def cpu(x):
    return x.cpu()


def wide(x):
    return x.to(torch_().int64)


def strided(x):
    """the same shape and values, every stride doubled: not contiguous, last stride 2"""
    t = torch_()
    return t.stack([x, x], dim=-1)[..., 0]


def shorter(x):
    return x.reshape(-1)[:-1]


def uneven(x):
    """[rows][mf][n] of the same values whose rows lie 2 mf packets apart"""
    t = torch_()
    big = t.cat([x, x], dim=1)                    # [rows][2 mf][n]: stride(0) = 2 mf stride(1)
    return big[:, :x.shape[1]]


def arg(name, change):
    """spoil the argument `name` by `change`"""
    return lambda a: a.__setitem__(name, change(a[name]))


def member(name, i, change):
    """spoil member i of the tuple argument `name`"""
    def apply(a):
        parts = list(a[name])
        parts[i] = change(parts[i])
        a[name] = tuple(parts)
    return apply


def to(name, value):
    return lambda a: a.__setitem__(name, value)


def both(*changes):
    def apply(a):
        for change in changes:
            change(a)
    return apply


def fewer(x):
    """[rows][mf - 1][n], evenly spaced"""
    rows, mf, n = x.shape
    return x.reshape(-1)[:rows * (mf - 1) * n].view(rows, mf - 1, n)


def same_as(name, i, other):
    """member i of the tuple `name` becomes the tensor of argument `other`"""
    return lambda a: member(name, i, lambda _: a[other])(a)


# (id, base call, the rule it hits, how)
CASES = [
    # marker_search
    ("marker-bytes-cpu", base_marker_search, "bytes: uint8 CUDA, one row or [rows][>= ceil(n_bits/8)], contiguous rows", arg("bytes", cpu)),
    ("marker-bytes-dtype", base_marker_search, "same", arg("bytes", wide)),
    ("marker-bytes-3d", base_marker_search, "same", arg("bytes", lambda x: x[None])),
    ("marker-bytes-strided", base_marker_search, "same", arg("bytes", strided)),
    ("marker-bytes-short", base_marker_search, "n_bits bits need ceil(n_bits/8) bytes per row", arg("bytes", lambda x: x[:, :NB - 1])),
    ("marker-period-0", base_marker_search, "period 1 .. 2^31 - 1", to("period", 0)),
    ("marker-period-2^31", base_marker_search, "same", to("period", 1 << 31)),
    ("marker-history-missing", base_marker_search, "history_bits > 0 needs the history words", to("history_bits", 5)),
    ("marker-history-count", base_marker_search, "history holds one word per row", both(to("history_bits", 5), to("history", [1, 2, 3]))),
    ("marker-history-tensor-count", base_marker_search, "same, as a tensor",
     both(to("history_bits", 5), lambda a: a.__setitem__("history", zeros32(3)))),
    ("marker-accumulate-alone", base_marker_search, "accumulate=True needs out", both(to("out", None), to("accumulate", True))),
    ("marker-out-cpu", base_marker_search, "out: contiguous int32 CUDA of [rows][period], [rows][period], [rows][4]", member("out", 0, cpu)),
    ("marker-out-dtype", base_marker_search, "same", member("out", 1, wide)),
    ("marker-out-strided", base_marker_search, "same", member("out", 1, strided)),
    ("marker-out-size", base_marker_search, "same", member("out", 2, shorter)),
    # frames_extract
    ("frames-bytes-cpu", base_frames_extract, "bytes: as marker_search", arg("bytes", cpu)),
    ("frames-bytes-dtype", base_frames_extract, "same", arg("bytes", wide)),
    ("frames-bytes-strided", base_frames_extract, "same", arg("bytes", strided)),
    ("frames-bytes-short", base_frames_extract, "n_bits bits need ceil(n_bits/8) bytes per row", arg("bytes", lambda x: x[:, :NB - 1])),
    ("frames-period-7", base_frames_extract, "period 8 .. 2^31 - 1, drop_bits below it, n_bits >= 1", to("period", 7)),
    ("frames-drop-bits", base_frames_extract, "same", to("drop_bits", PERIOD)),
    ("frames-n-bits-0", base_frames_extract, "same", to("n_bits", 0)),
    ("frames-lock-cpu", base_frames_extract, "lock: contiguous int32 CUDA [rows][4]", arg("lock", cpu)),
    ("frames-lock-dtype", base_frames_extract, "same", arg("lock", wide)),
    ("frames-lock-strided", base_frames_extract, "same", arg("lock", strided)),
    ("frames-lock-size", base_frames_extract, "same", arg("lock", lambda x: x[:1])),
    ("frames-out0-cpu", base_frames_extract, "out[0]: uint8 CUDA [rows][max_frames][>= ceil(Q/8)], evenly spaced", member("out", 0, cpu)),
    ("frames-out0-2d", base_frames_extract, "same", member("out", 0, lambda x: x.reshape(ROWS * CAP, QB))),
    ("frames-out0-max-frames", base_frames_extract, "same", member("out", 0, lambda x: x[:, :CAP - 1])),
    ("frames-out0-narrow", base_frames_extract, "same", member("out", 0, lambda x: x[..., :QB - 1])),
    ("frames-out0-strided", base_frames_extract, "same", member("out", 0, strided)),
    ("frames-out0-uneven", base_frames_extract, "same", member("out", 0, uneven)),
    ("frames-n-frames-cpu", base_frames_extract, "out[1], out[2], out[4]: contiguous int32 CUDA", member("out", 1, cpu)),
    ("frames-marker-errors-size", base_frames_extract, "same", member("out", 2, shorter)),
    ("frames-carry-bits-out-dtype", base_frames_extract, "same", member("out", 4, wide)),
    ("frames-carry-out-cpu", base_frames_extract, "a carry: uint8 CUDA [rows][>= ceil((period-1)/8)], contiguous rows", member("out", 3, cpu)),
    ("frames-carry-out-narrow", base_frames_extract, "same", member("out", 3, lambda x: x[:, :CB - 1])),
    ("frames-carry-rows", base_frames_extract, "same", arg("carry", lambda x: x[:1])),
    ("frames-carry-strided", base_frames_extract, "same", arg("carry", strided)),
    ("frames-carry-dtype", base_frames_extract, "same", arg("carry", wide)),
    ("frames-carry-bits-missing", base_frames_extract, "carry needs carry_bits, contiguous int32 CUDA [rows]", to("carry_bits", None)),
    ("frames-carry-bits-cpu", base_frames_extract, "same", arg("carry_bits", cpu)),
    ("frames-carry-bits-size", base_frames_extract, "same", arg("carry_bits", lambda x: x[:1])),
    ("frames-carry-is-carry-out", base_frames_extract, "carry and carry_out distinct", same_as("out", 3, "carry")),
    ("frames-carry-stride", base_frames_extract, "carry and carry_out of one row stride",
     arg("carry", lambda x: torch_().cat([x, x], dim=1)[:, :CB])),
    ("frames-pad-cpu", base_frames_extract, "pad: contiguous uint8 CUDA of >= ceil(Q/8) bytes", arg("pad", cpu)),
    ("frames-pad-strided", base_frames_extract, "same", arg("pad", strided)),
    ("frames-pad-short", base_frames_extract, "same", arg("pad", lambda x: x[:QB - 1])),
    # rs_decode, DVB (204,188) I = 1 and CCSDS (255,223) I = 2
    ("rs-frames-cpu", base_rs_decode, "frames: uint8 CUDA [rows][max_frames][>= n I] or [max_frames][...]", both(arg("frames", cpu), to("out", None))),
    ("rs-frames-dtype", base_rs_decode, "same", both(arg("frames", wide), to("out", None))),
    ("rs-frames-1d", base_rs_decode, "same", both(arg("frames", lambda x: x.reshape(-1)), to("out", None))),
    ("rs-frames-strided", base_rs_decode, "same", both(arg("frames", strided), to("out", None))),
    ("rs-interleave-0", base_rs_decode, "interleave >= 1 and n I bytes fit the last dimension", to("interleave", 0)),
    ("rs-frames-narrow", base_rs_decode_ccsds, "same", both(arg("frames", lambda x: x[..., :509]), arg("out", lambda x: x[..., :509]))),
    ("rs-frames-narrow-dvb", base_rs_decode, "same", to("interleave", 2)),
    ("rs-frames-uneven", base_rs_decode_ccsds, "frames evenly spaced", both(arg("frames", uneven), to("out", None))),
    ("rs-out-cpu", base_rs_decode, "out: uint8 CUDA with the shape and strides of frames", arg("out", cpu)),
    ("rs-out-dtype", base_rs_decode, "same", arg("out", wide)),
    ("rs-out-shape", base_rs_decode_ccsds, "same", arg("out", lambda x: x[:, :MF - 1])),
    ("rs-out-strides", base_rs_decode, "same", arg("out", uneven)),
    ("rs-n-frames-cpu", base_rs_decode, "n_frames: contiguous int32 CUDA [rows]", arg("n_frames", cpu)),
    ("rs-n-frames-dtype", base_rs_decode_ccsds, "same", arg("n_frames", wide)),
    ("rs-n-frames-strided", base_rs_decode, "same", arg("n_frames", strided)),
    ("rs-n-frames-size", base_rs_decode, "same", arg("n_frames", lambda x: x[:1])),
    ("rs-status-cpu", base_rs_decode, "status: contiguous int32 CUDA of rows max_frames I entries", arg("status", cpu)),
    ("rs-status-dtype", base_rs_decode, "same", arg("status", wide)),
    ("rs-status-strided", base_rs_decode_ccsds, "same", arg("status", strided)),
    ("rs-status-size", base_rs_decode_ccsds, "same", arg("status", lambda x: x[..., :1])),
    # deinterleave: the packet rule, the count rule, the history rule
    ("deint-packets-cpu", base_deinterleave, "packets: uint8 CUDA [rows][max_frames][>= n] or [max_frames][...]", arg("packets", cpu)),
    ("deint-packets-dtype", base_deinterleave, "same", arg("packets", wide)),
    ("deint-packets-1d", base_deinterleave, "same", arg("packets", lambda x: x.reshape(-1))),
    ("deint-packets-strided", base_deinterleave, "same", both(arg("packets", strided), to("packet_bytes", PACKET))),
    ("deint-packets-narrow", base_deinterleave, "same", both(arg("packets", lambda x: x[..., :PACKET - 12]), to("packet_bytes", PACKET))),
    ("deint-packets-uneven", base_deinterleave, "packets evenly spaced", arg("packets", uneven)),
    ("deint-branches-1", base_deinterleave, "branches >= 2, cell >= 1, packet_bytes a multiple of branches", to("branches", 1)),
    ("deint-cell-0", base_deinterleave, "same", to("cell", 0)),
    ("deint-packet-bytes", base_deinterleave, "same", to("packet_bytes", 200)),
    ("deint-out0-cpu", base_deinterleave, "out[0]: the packet rule", member("out", 0, cpu)),
    ("deint-out0-uneven", base_deinterleave, "out[0] evenly spaced", member("out", 0, uneven)),
    ("deint-out0-shape", base_deinterleave, "out[0] holds [rows][max_frames] packets", member("out", 0, fewer)),
    ("deint-n-frames-cpu", base_deinterleave, "n_frames, out[1], out[3]: contiguous int32 CUDA [rows]", arg("n_frames", cpu)),
    ("deint-n-out-dtype", base_deinterleave, "same", member("out", 1, wide)),
    ("deint-fill-out-size", base_deinterleave, "same", member("out", 3, lambda x: x[:1])),
    ("deint-fill-out-strided", base_deinterleave, "same", member("out", 3, strided)),
    ("deint-hist-out-cpu", base_deinterleave, "a history: uint8 CUDA [rows][>= H n], contiguous rows", member("out", 2, cpu)),
    ("deint-hist-out-narrow", base_deinterleave, "same", member("out", 2, lambda x: x[:, :H * PACKET - 1])),
    ("deint-hist-rows", base_deinterleave, "same", arg("hist", lambda x: x[:1])),
    ("deint-hist-strided", base_deinterleave, "same", arg("hist", strided)),
    ("deint-hist-dtype", base_deinterleave, "same", arg("hist", wide)),
    ("deint-fill-missing", base_deinterleave, "hist needs fill", to("fill", None)),
    ("deint-fill-cpu", base_deinterleave, "fill: contiguous int32 CUDA [rows]", arg("fill", cpu)),
    ("deint-hist-is-hist-out", base_deinterleave, "hist and hist_out distinct", same_as("out", 2, "hist")),
    ("deint-hist-stride", base_deinterleave, "hist and hist_out of one row stride",
     arg("hist", lambda x: torch_().cat([x, x], dim=1)[:, :H * PACKET])),
    # dvb_derandomize
    ("dvb-packets-cpu", base_dvb_derandomize, "packets: the packet rule, >= 188 bytes", arg("packets", cpu)),
    ("dvb-packets-narrow", base_dvb_derandomize, "same", arg("packets", lambda x: x[..., :187])),
    ("dvb-packets-uneven", base_dvb_derandomize, "packets evenly spaced", arg("packets", uneven)),
    ("dvb-in-place-and-out", base_dvb_derandomize, "in_place=True takes no out", to("in_place", True)),
    ("dvb-out-cpu", base_dvb_derandomize, "out: the packet rule", arg("out", cpu)),
    ("dvb-out-narrow", base_dvb_derandomize, "same", arg("out", lambda x: x[..., :187])),
    ("dvb-out-shape", base_dvb_derandomize, "out holds [rows][max_frames] packets", arg("out", fewer)),
    ("dvb-n-frames-dtype", base_dvb_derandomize, "n_frames, phase, phase_out: contiguous int32 CUDA [rows]", arg("n_frames", wide)),
    ("dvb-phase-cpu", base_dvb_derandomize, "same", arg("phase", cpu)),
    ("dvb-phase-out-size", base_dvb_derandomize, "same", arg("phase_out", lambda x: x[:1])),
    ("dvb-sync-errors-cpu", base_dvb_derandomize, "sync_errors, rs_status: contiguous int32 CUDA of rows max_frames entries", arg("sync_errors", cpu)),
    ("dvb-sync-errors-strided", base_dvb_derandomize, "same", arg("sync_errors", strided)),
    ("dvb-rs-status-dtype", base_dvb_derandomize, "same", arg("rs_status", wide)),
    ("dvb-rs-status-size", base_dvb_derandomize, "same", arg("rs_status", lambda x: x[:, :MF - 1])),
    # encode / channel_errors: the shared byte and start-state rules, then each one's own
    ("encode-tail-biting-start", base_encode, "a tail-biting frame takes no start_state", both(to("tail_biting", True), to("start_state", [0, 0]))),
    ("encode-bytes-cpu", base_encode, "bytes: uint8 CUDA, 1-D or 2-D, contiguous rows", arg("bytes", cpu)),
    ("encode-bytes-dtype", base_encode, "same", arg("bytes", wide)),
    ("encode-bytes-3d", base_encode, "same", arg("bytes", lambda x: x[None])),
    ("encode-bytes-strided", base_encode, "same", arg("bytes", strided)),
    ("encode-bytes-narrow", base_encode, "L bits need ceil(L/8) bytes per frame", arg("bytes", lambda x: x[:, :L // 8 - 1])),
    ("encode-bytes-no-frame", base_encode, "bytes holds no frame", arg("bytes", lambda x: x.reshape(-1)[:L // 8 - 1])),
    ("encode-bytes-no-rows", base_encode, "same", arg("bytes", lambda x: x[:0])),
    ("encode-start-state-count", base_encode, "start_state holds one state per frame", to("start_state", [0, 1, 2])),
    ("encode-out-cpu", base_encode, "out: soft dtype, CUDA", arg("out", cpu)),
    ("encode-out-dtype", base_encode, "same", arg("out", wide)),
    ("encode-out-size", base_encode, "out holds frames x steps R symbols, or [frames][>= steps R] rows", arg("out", shorter)),
    ("encode-out-strided", base_encode, "same", arg("out", strided)),
    ("encode-end-state-cpu", base_encode, "end_state_out: contiguous int32 CUDA [frames]", arg("end_state_out", cpu)),
    ("encode-end-state-dtype", base_encode, "same", arg("end_state_out", wide)),
    ("encode-end-state-strided", base_encode, "same", arg("end_state_out", strided)),
    ("encode-end-state-size", base_encode, "same", arg("end_state_out", lambda x: x[:1])),
    ("errors-tail-biting-start", base_channel_errors, "a tail-biting frame takes no start_state", both(to("tail_biting", True), to("start_state", [0, 0]))),
    ("errors-bytes-cpu", base_channel_errors, "bytes: as encode", arg("bytes", cpu)),
    ("errors-bytes-stride", base_channel_errors, "bytes holds no frame at a stride below ceil(L/8)", to("bytes_frame_stride", L // 8 - 1)),
    ("errors-start-state-count", base_channel_errors, "start_state holds one state per frame", to("start_state", [0])),
    ("errors-symbols-cpu", base_channel_errors, "symbols: soft dtype, CUDA, last dimension contiguous", arg("symbols", cpu)),
    ("errors-symbols-dtype", base_channel_errors, "same", arg("symbols", wide)),
    ("errors-symbols-strided", base_channel_errors, "same", arg("symbols", strided)),
    ("errors-symbols-layout", base_channel_errors, "symbols hold frames x steps R, or pass symbol_frame_stride", arg("symbols", lambda x: x[:1])),
    ("errors-symbols-room", base_channel_errors, "frames at that stride fit the symbol tensor", to("symbol_frame_stride", 10 * (L + 6))),
    ("errors-symbols-stride-small", base_channel_errors, "same", to("symbol_frame_stride", L)),
    # update_resume
    ("resume-symbols-cpu", base_update_resume, "symbols: soft dtype, CUDA", arg("symbols", cpu)),
    ("resume-symbols-dtype", base_update_resume, "same", arg("symbols", wide)),
    ("resume-symbols-strided", base_update_resume, "packed chunks contiguous", arg("symbols", strided)),
    ("resume-metrics-shape", base_update_resume, "metrics: contiguous [frames][N]", arg("metrics", lambda x: x[:, :32])),
    ("resume-metrics-strided", base_update_resume, "same", arg("metrics", strided)),
    ("resume-symbols-frames", base_update_resume, "packed chunks are [frames][n_steps][R]", arg("symbols", lambda x: x[:1])),
    ("resume-symbols-few", base_update_resume, "symbols cover the last frame's chunk", to("n_steps", L + 7)),
    # decode_stream / decode_streams
    ("stream-symbols-cpu", base_decode_stream, "symbols: contiguous soft dtype CUDA of [steps][R]", arg("symbols", cpu)),
    ("stream-symbols-dtype", base_decode_stream, "same", arg("symbols", wide)),
    ("stream-symbols-strided", base_decode_stream, "same", arg("symbols", strided)),
    ("stream-symbols-odd", base_decode_stream, "same", arg("symbols", shorter)),
    ("stream-rule", base_decode_stream, "head, tail >= K-1, window >= 8, head, tail, a segment that emits bits", to("head", 5)),
    ("stream-rule-window", base_decode_stream, "same", to("window", 40)),
    ("stream-workspace", base_decode_stream, "workspace large enough and 256-byte aligned", lambda a: a.__setitem__("workspace", poisoned((256,), torch_().uint8))),
    ("stream-out-cpu", base_decode_stream, "out: contiguous uint8 CUDA of ceil(n_bits/8) elements", arg("out", cpu)),
    ("stream-out-dtype", base_decode_stream, "same", arg("out", wide)),
    ("stream-out-strided", base_decode_stream, "same", arg("out", strided)),
    ("stream-out-size", base_decode_stream, "same", arg("out", shorter)),
    ("streams-symbols-cpu", base_decode_streams, "symbols: contiguous soft dtype CUDA of [n_streams][pitch][R]", arg("symbols", cpu)),
    ("streams-symbols-dtype", base_decode_streams, "same", arg("symbols", wide)),
    ("streams-symbols-strided", base_decode_streams, "same", arg("symbols", strided)),
    ("streams-symbols-2d", base_decode_streams, "same", arg("symbols", lambda x: x.reshape(ROWS, -1))),
    ("streams-rule-pitch", base_decode_streams, "what decode_stream needs, pitch >= steps, pitch a multiple of the window",
     arg("symbols", lambda x: x[:, :PITCH - 1].contiguous())),
    ("streams-rule-steps", base_decode_streams, "same", to("steps", PITCH + 1)),
    ("streams-out-cpu", base_decode_streams, "out: uint8 CUDA [n_streams][>= ceil(n_bits/8)], contiguous rows", arg("out", cpu)),
    ("streams-out-dtype", base_decode_streams, "same", arg("out", wide)),
    ("streams-out-1d", base_decode_streams, "same", arg("out", lambda x: x.reshape(-1))),
    ("streams-out-rows", base_decode_streams, "same", arg("out", lambda x: x[:1])),
    ("streams-out-narrow", base_decode_streams, "same", arg("out", lambda x: x[:, :EMITTED - 1])),
    ("streams-out-strided", base_decode_streams, "same", arg("out", strided)),
    ("streams-out-overlap", base_decode_streams, "same", arg("out", lambda x: x[:1].expand(ROWS, EMITTED))),
    # decode_tail_biting
    ("tb-symbols-cpu", base_decode_tail_biting, "symbols: contiguous soft dtype CUDA", arg("symbols", cpu)),
    ("tb-symbols-dtype", base_decode_tail_biting, "same", arg("symbols", wide)),
    ("tb-symbols-strided", base_decode_tail_biting, "same", arg("symbols", strided)),
    ("tb-symbols-shape", base_decode_tail_biting, "symbols are [frames][n_steps][R]", to("L", L - 1)),
    ("tb-rule", base_decode_tail_biting, "L >= K and head, tail >= K-1", to("head", 5)),
    ("tb-workspace-small", base_decode_tail_biting, "workspace large enough and 256-byte aligned",
     lambda a: a.__setitem__("workspace", poisoned((256,), torch_().uint8))),
    ("tb-workspace-unaligned", base_decode_tail_biting, "same", lambda a: a.__setitem__("workspace", poisoned((1 << 20,), torch_().uint8)[1:])),
    ("tb-out-cpu", base_decode_tail_biting, "out, end_state_out, ok_out: contiguous CUDA of their dtype and size", arg("out", cpu)),
    ("tb-out-size", base_decode_tail_biting, "same", arg("out", shorter)),
    ("tb-end-state-dtype", base_decode_tail_biting, "same", arg("end_state_out", wide)),
    ("tb-ok-strided", base_decode_tail_biting, "same", arg("ok_out", strided)),
    # sync_build
    ("sync-received-cpu", base_sync_build, "received: contiguous 1-D soft dtype CUDA", arg("received", cpu)),
    ("sync-received-dtype", base_sync_build, "same", arg("received", wide)),
    ("sync-received-2d", base_sync_build, "same", arg("received", lambda x: x.reshape(2, -1))),
    ("sync-received-strided", base_sync_build, "same", arg("received", strided)),
    ("sync-no-hypothesis", base_sync_build, "1 to 64 hypotheses", both(to("hypotheses", []), to("out", None))),
    ("sync-65-hypotheses", base_sync_build, "same", both(to("hypotheses", [(0, 0)] * 65), to("out", None))),
    ("sync-mask-odd", base_sync_build, "the mask covers whole steps and keeps a symbol", to("mask", [1, 1, 1])),
    ("sync-mask-empty", base_sync_build, "same", to("mask", [])),
    ("sync-mask-none-kept", base_sync_build, "same", to("mask", [0, 0, 0, 0])),
    ("sync-out-cpu", base_sync_build, "out: contiguous soft dtype CUDA of [n_hyp][pitch][R]", arg("out", cpu)),
    ("sync-out-dtype", base_sync_build, "same", arg("out", wide)),
    ("sync-out-strided", base_sync_build, "same", arg("out", strided)),
    ("sync-out-size", base_sync_build, "same", to("pitch", L + 1)),
    # depuncture
    ("depuncture-mask-odd", base_depuncture, "the puncturing vector covers whole steps", to("mask", [1, 1, 1])),
    ("depuncture-cpu", base_depuncture, "punctured: contiguous [frames][P] device tensor", arg("punctured", cpu)),
    ("depuncture-1d", base_depuncture, "same", arg("punctured", lambda x: x.reshape(-1))),
    ("depuncture-strided", base_depuncture, "same", arg("punctured", strided)),
    ("depuncture-dtype", base_depuncture, "punctured: the soft dtype, sum(mask) symbols per frame", arg("punctured", wide)),
    ("depuncture-count", base_depuncture, "same", arg("punctured", lambda x: x[:, :23].contiguous())),
]


def tensors_of(args):
    t = torch_()
    for value in args.values():
        for x in (value if isinstance(value, (tuple, list)) else (value,)):
            if t.is_tensor(x):
                yield x


def snapshot(xs):
    return [x.cpu().clone() for x in xs]


@pytest.mark.parametrize("base,rule,spoil", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_a_spoiled_argument_is_rejected_before_any_launch(base, rule, spoil):
    t = torch_()
    call, args = base()
    held = list(tensors_of(args))
    spoil(args)
    held += [x for x in tensors_of(args) if not any(x is y for y in held)]
    before = snapshot(held)
    t.cuda.synchronize()
    with pytest.raises(ValueError):
        call(**args)
    t.cuda.synchronize()
    for x, was in zip(held, before):
        assert t.equal(x.cpu(), was), rule


def test_every_base_call_is_accepted_and_writes_its_outputs():
    """the calls the cases start from pass as they stand (so each case fails for its own reason), and an output that was 0xA5 is written"""
    t = torch_()
    for base in (base_marker_search, base_frames_extract, base_rs_decode, base_rs_decode_ccsds, base_deinterleave, base_dvb_derandomize,
                 base_encode, base_channel_errors, base_update_resume, base_decode_stream, base_decode_streams, base_decode_tail_biting,
                 base_sync_build, base_depuncture):
        call, args = base()
        call(**args)
        t.cuda.synchronize()
        out = args["status"] if "status" in args else args.get("out")       # an uncorrectable word is left as received: see its status
        for x in (out if isinstance(out, tuple) else (out,)):
            if x is not None and (x.numel() > 8 or "status" in args):
                assert not bool((x.contiguous().view(t.uint8) == 0xA5).all()), base.__name__


def run(base, **changes):
    """the base call with `changes`; every tensor it returned, on the host"""
    t = torch_()
    call, args = base()
    for name, value in changes.items():
        args[name] = value(args) if callable(value) else value
    got = call(**args)
    t.cuda.synchronize()
    return [x.cpu().numpy() for x in (got if isinstance(got, tuple) else (got,)) if t.is_tensor(x)]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x.reshape(-1), y.reshape(-1))


def written(got):
    """of what frames_extract returned, the parts it wrote: the counts, each row's frames and marker errors, its carry bytes"""
    frames, n, errors, carry, bits = got
    rows = len(n)
    frames, errors, carry = frames.reshape(rows, -1, frames.shape[-1]), errors.reshape(rows, -1), carry.reshape(rows, -1)
    return [n, bits] + [part for r in range(rows) for part in (frames[r, :n[r], :QB], errors[r, :n[r]], carry[r, :(bits[r] + 7) // 8])]


def outcome(base, **changes):
    """what run() gives, or the error the C ABI answers with once the host rules have let the call through"""
    try:
        return run(base, **changes)
    except _lib.VitHipError as e:
        return str(e)


def test_edge_an_empty_bytes_tensor_may_have_any_stride():
    """marker_search with n_bits = 0 and the whole marker in the history.  The host rule does not look at an empty tensor's strides:
    no ValueError, the call reaches the C ABI.  torch gives an empty tensor a NULL address, which the C ABI turns down -- with the
    same words for the plain layout and the strided one"""
    kw = dict(n_bits=0, history=[MARKER, 0x12], history_bits=8, out=None)
    plain = outcome(base_marker_search, bytes=lambda a: a["bytes"][:, :0], **kw)
    odd = outcome(base_marker_search, bytes=lambda a: a["bytes"][:, 0:0:2], **kw)
    assert plain == odd if isinstance(plain, str) else same(plain, odd) is None
    assert not isinstance(plain, str) or "NULL buffer" in plain


def test_edge_an_empty_frames_tensor_may_have_any_stride():
    """rs_decode on [rows][0][n]: the packet rule lets it through whatever the strides say (no ValueError); the C ABI answers the plain
    layout and the strided one alike, and nothing is written"""
    t = torch_()
    status = poisoned((ROWS, MF, 1), t.int32)
    got = [outcome(base_rs_decode, frames=frames, out=None, status=status[:, :0])
           for frames in (lambda a: a["frames"][:, :0], lambda a: t.cat([a["frames"], a["frames"]], dim=2)[:, :0, ::2])]
    if isinstance(got[0], str):
        assert got[0] == got[1] and "NULL" in got[0]
    else:
        assert all(g[0].shape == (ROWS, 0, PACKET) and g[1].shape == (ROWS, 0, 1) for g in got)
    assert bool((status.view(t.uint8) == 0xA5).all())


def test_edge_one_row_is_one_or_two_dimensional():
    one = lambda name: (lambda a: a[name][0])                  # noqa: E731
    two = lambda name: (lambda a: a[name][:1])                 # noqa: E731
    kw = dict(out=None)
    same(run(base_marker_search, bytes=one("bytes"), **kw), run(base_marker_search, bytes=two("bytes"), **kw))
    kw = dict(out=None, carry=None, carry_bits=None, lock=lambda a: a["lock"][:1])
    same(written(run(base_frames_extract, bytes=one("bytes"), **kw)), written(run(base_frames_extract, bytes=two("bytes"), **kw)))
    kw = dict(out=None, status=None, n_frames=lambda a: a["n_frames"][:1])
    same(run(base_rs_decode, frames=one("frames"), **kw), run(base_rs_decode, frames=two("frames"), **kw))
    same(run(base_rs_decode_ccsds, frames=one("frames"), **kw), run(base_rs_decode_ccsds, frames=two("frames"), **kw))
    kw = dict(out=None, hist=lambda a: a["hist"][:1], fill=lambda a: a["fill"][:1], n_frames=lambda a: a["n_frames"][:1])
    same(run(base_deinterleave, packets=one("packets"), **kw), run(base_deinterleave, packets=two("packets"), **kw))
    kw = dict(out=None, phase=None, rs_status=None, phase_out=None, sync_errors=None, n_frames=lambda a: a["n_frames"][:1])
    same(run(base_dvb_derandomize, packets=one("packets"), **kw), run(base_dvb_derandomize, packets=two("packets"), **kw))


def test_edge_a_frames_tensor_may_be_wider():
    """the last stride is the frame stride: the bytes behind a frame are neither read nor written"""
    t = torch_()
    guard = 6

    def wider(name, n):
        def make(a):
            x = poisoned(tuple(a[name].shape[:-1]) + (n + guard,), t.uint8)
            x[..., :n] = a[name]
            return x
        return make

    plain = run(base_rs_decode, out=None, status=None)
    wide_ = run(base_rs_decode, frames=wider("frames", PACKET), out=None, status=None)
    assert np.array_equal(wide_[0][..., :PACKET], plain[0]) and (wide_[0][..., PACKET:] == 0xA5).all() and np.array_equal(wide_[1], plain[1])
    plain = run(base_rs_decode_ccsds, out=None, status=None)
    wide_ = run(base_rs_decode_ccsds, frames=wider("frames", 510), out=None, status=None)
    assert np.array_equal(wide_[0][..., :510], plain[0]) and (wide_[0][..., 510:] == 0xA5).all() and np.array_equal(wide_[1], plain[1])
    # frames_extract writes into a wider out[0]; deinterleave and dvb_derandomize read wider packets
    plain = run(base_frames_extract)
    wide_ = run(base_frames_extract, out=lambda a: (poisoned((ROWS, CAP, QB + guard), t.uint8),) + a["out"][1:])
    assert (wide_[0][..., QB:] == 0xA5).all()
    n = plain[1]
    for r in range(ROWS):
        assert np.array_equal(wide_[0][r, :n[r], :QB], plain[0][r, :n[r]])
    same(wide_[1:], plain[1:])
    same(run(base_deinterleave, packets=wider("packets", PACKET), packet_bytes=PACKET), run(base_deinterleave))
    same(run(base_dvb_derandomize, packets=wider("packets", PACKET)), run(base_dvb_derandomize))


def test_edge_a_single_row_may_have_any_row_stride():
    """rows = 1: stride(0) is never used, so a row cut out of a larger tensor is as good as its copy"""
    t = torch_()
    cut = lambda name: (lambda a: t.cat([a[name][:1]] * 5)[::5])                      # noqa: E731  [1][...] with stride(0) = 5 rows
    copy = lambda name: (lambda a: a[name][:1].clone())                                # noqa: E731
    head = lambda name: (lambda a: a[name][:1])                                        # noqa: E731
    assert cut("x")({"x": t.zeros(2, 3, 4)}).stride(0) == 60
    kw = dict(out=None)
    same(run(base_marker_search, bytes=cut("bytes"), **kw), run(base_marker_search, bytes=copy("bytes"), **kw))
    kw = dict(out=None, carry=None, carry_bits=None, lock=head("lock"))
    same(written(run(base_frames_extract, bytes=cut("bytes"), **kw)), written(run(base_frames_extract, bytes=copy("bytes"), **kw)))
    kw = dict(out=None, status=None, n_frames=head("n_frames"))
    same(run(base_rs_decode, frames=cut("frames"), **kw), run(base_rs_decode, frames=copy("frames"), **kw))
    kw = dict(out=None, hist=head("hist"), fill=head("fill"), n_frames=head("n_frames"))
    same(run(base_deinterleave, packets=cut("packets"), **kw), run(base_deinterleave, packets=copy("packets"), **kw))
    # a carry / history row of a single-row call: its width is its stride, whatever stride(0) says
    kw = dict(out=None, lock=head("lock"), bytes=head("bytes"), carry_bits=head("carry_bits"))
    same(written(run(base_frames_extract, carry=cut("carry"), **kw)), written(run(base_frames_extract, carry=copy("carry"), **kw)))
