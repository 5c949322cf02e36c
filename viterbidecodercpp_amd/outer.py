"""The outer chain of a receiver on the GPU, behind the Viterbi decoder: frame marker search, frame extraction, Reed-Solomon decoding,
the convolutional de-interleaver, DVB-S energy-dispersal removal, the frame check (CRC), DAB energy-dispersal removal and the DAB+
superframe sync and access-unit table -- the routes of the C ABI that work on the caller's bytes alone and read the handle only for its
device (csrc/vit_marker.hip, vit_frames.hip, vit_rs.hip, vit_dvb.hip, vit_crc.hip, vit_dab.hip, vit_dabplus.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args, _lib


def _ptr(x):
    """the address a tensor starts at, as the C ABI takes it; NULL for None"""
    return None if x is None else C.c_void_p(x.data_ptr())


class _RsCode:
    """a vit_hip_rs_code: the tables of one reed_solomon.RSCode on the device of a handle, which it keeps alive"""

    def __init__(self, handle, code):
        self._handle = handle
        self._c = C.c_void_p()
        params = _lib.VitHipRsParams(code.gfpoly, code.fcr, code.prim, code.nroots, code.pad, int(code.dual_basis))
        _lib.check(_lib.load().vit_hip_rs_create(handle._h, C.byref(params), C.byref(self._c)))

    def __del__(self):
        try:
            if getattr(self, "_c", None):
                _lib.load().vit_hip_rs_destroy(self._c)
                self._c = None
        except Exception:
            pass


class _OuterChain:
    """The outer-chain methods of BatchDecoder, as a mix-in.  Of the class they are mixed into they use exactly: `torch` (the module),
    `device` (the torch.device), `_handle` (the _Handle of the decoder), `_stream()` (the current stream as the C ABI takes it) and
    `_rs_codes` (a dict, RSCode -> _RsCode: a code's tables are uploaded once per decoder)."""

    def _empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    def marker_search(self, bytes, n_bits: int, marker: int, marker_bits: int, period: int, phase0: int = 0, history=None,
                      history_bits: int = 0, out=None, accumulate=False):
        """frame synchronisation (vit_hip_marker_search): the Hamming distance of the sync marker (`marker_bits` bits, the first
        transmitted in the highest; frame_sync.CCSDS_ASM, DVB_SYNC) to every bit position of the decoded `bytes` -- uint8 CUDA, one
        row or [rows][>= ceil(n_bits/8)] with its row stride, MSB-first as the decode calls write them --, summed per phase of the
        frame period: position p belongs to phase (phase0 + p) mod period.  history [rows] (ints or a tensor): the `history_bits`
        <= 63 stream bits in front of bit 0, the latest in bit 0, so that positions straddling two calls are counted.  returns
        (distance, count, lock): int32 CUDA tensors [rows][period], [rows][period] and [rows][4] = (phase, inverted, errors,
        compared) of the candidate with the lowest errors / compared (compared = marker_bits * count; inverted: errors = compared -
        distance; the lower phase, then upright, on a tie).  out = (distance, count, lock) reuses those tensors; with
        accumulate=True the call adds to the totals they hold and the lock is that of the totals.  Nothing is copied to the host."""
        t = self.torch
        n_bits, period = int(n_bits), int(period)
        rows, stride = _args.bit_rows(bytes, n_bits)
        if period < 1 or period >= 1 << 31:
            raise ValueError("period must be 1 .. 2^31 - 1")
        hist = None
        if history_bits:
            if history is None:
                raise ValueError("history_bits > 0 needs the history words")
            if t.is_tensor(history):
                hist = history.to(device=self.device, dtype=t.int64).reshape(-1).contiguous()
            else:
                words = np.asarray([int(x) for x in np.asarray(history, dtype=object).reshape(-1)], dtype=np.uint64)
                hist = t.from_numpy(words.view(np.int64)).to(self.device)
            if hist.numel() != rows:
                raise ValueError("history must hold one word per row")
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True adds to the totals of out=(distance, count, lock)")
            out = (self._empty((rows, period), t.int32), self._empty((rows, period), t.int32), self._empty((rows, 4), t.int32))
        distance, count, lock = out
        for x, n, what in ((distance, period, "out[0]"), (count, period, "out[1]"), (lock, 4, "out[2]")):
            _args.dense(x, t.int32, rows * n, what)
        _lib.check(_lib.load().vit_hip_marker_search(
            self._handle._h, _ptr(bytes), stride, rows, n_bits, int(marker), int(marker_bits), _ptr(hist), int(history_bits), period,
            int(phase0), _lib.MARKER_ACCUMULATE if accumulate else 0, _ptr(distance), _ptr(count), _ptr(lock), self._stream()))
        return distance, count, lock

    def frames_capacity(self, n_bits: int, period: int) -> int:
        """the most frames one frames_extract call over n_bits bits per row can complete: ceil(n_bits / period)"""
        return int(_lib.load().vit_hip_frames_capacity(int(n_bits), int(period)))

    def frames_extract(self, bytes, n_bits: int, period: int, phase0: int, lock, carry=None, carry_bits=None, marker: int = 0,
                       marker_bits: int = 0, drop_bits: int = 0, pad=None, max_frames: int = None, out=None):
        """frame extraction (vit_hip_frames_extract): the frames of the decoded `bytes` -- uint8 CUDA, one row or [rows][>=
        ceil(n_bits/8)], MSB-first, bit 0 at phase `phase0` of the frame period -- cut at `lock`, the int32 [rows][4] tensor
        marker_search returns (read on the device: phase and inverted).  carry / carry_bits: the uint8 [rows][>= ceil((period-1)/8)]
        and int32 [rows] the previous call returned as carry_out / carry_bits_out (None: nothing carried).  A frame is complemented
        under an inverted lock, loses its first `drop_bits` bits (the marker) and is XORed with `pad`, uint8 CUDA [ceil(Q/8)] for its Q
        = period - drop_bits output bits (frame_sync.ccsds_randomizer; None: none).  returns (frames, n_frames, marker_errors,
        carry_out, carry_bits_out): uint8 [rows][max_frames][ceil(Q/8)] of which the first n_frames[r] (int32 [rows]) of row r are
        written, int32 [rows][max_frames] = the bits of `marker` (marker_bits <= 64; 0: off, and None is returned) each written frame
        differs in, and the unfinished frame's raw bits with their number.  max_frames defaults to frames_capacity(n_bits, period).
        out = the same five reuses those tensors (frames may have a larger last dimension: its stride is the frame stride); carry
        and carry_out must be distinct and have the same row stride.  Nothing is copied to the host."""
        t = self.torch
        n_bits, period, drop_bits, marker_bits = int(n_bits), int(period), int(drop_bits), int(marker_bits)
        rows, stride = _args.bit_rows(bytes, n_bits)
        if not 8 <= period < 1 << 31 or not 0 <= drop_bits < period or n_bits < 1:
            raise ValueError("period must be 8 .. 2^31 - 1, drop_bits below it, n_bits at least 1")
        qb, cb = (period - drop_bits + 7) // 8, (period - 1 + 7) // 8
        max_frames = self.frames_capacity(n_bits, period) if max_frames is None else int(max_frames)
        _args.dense(lock, t.int32, rows * 4, "lock")
        if out is None:
            out = (self._empty((rows, max_frames, qb), t.uint8), self._empty(rows, t.int32),
                   self._empty((rows, max_frames), t.int32) if marker_bits else None, self._empty((rows, cb), t.uint8), self._empty(rows, t.int32))
        frames, n_frames, marker_errors, carry_out, carry_bits_out = out
        # stricter than the packet rule: three dimensions, the rows and max_frames of this call, and no leave for an empty tensor
        if (_args.device(frames, t.uint8, "out[0]").dim() != 3 or tuple(frames.shape[:2]) != (rows, max_frames) or frames.shape[2] < qb
                or frames.stride(2) != 1 or (rows > 1 and frames.stride(0) != max_frames * frames.stride(1))):
            raise ValueError(f"out[0] must be [{rows}][{max_frames}][>= {qb}] with evenly spaced frames")
        for x, n, what in ((n_frames, rows, "out[1]"), (marker_errors, rows * max_frames, "out[2]"), (carry_bits_out, rows, "out[4]")):
            if x is not None:
                _args.dense(x, t.int32, n, what)
        cstride = _args.carried(carry, carry_bits, carry_out, rows, cb, "carry", "carry_bits")
        if pad is not None and _args.dense(pad, t.uint8, None, "pad").numel() < qb:
            raise ValueError(f"pad must hold at least {qb} bytes")
        _lib.check(_lib.load().vit_hip_frames_extract(
            self._handle._h, _ptr(bytes), stride, rows, n_bits, period, int(phase0), _ptr(lock), _ptr(carry),
            _ptr(carry_bits) if carry is not None else None, cstride, int(marker), marker_bits, drop_bits, _ptr(pad), _ptr(frames),
            int(frames.stride(1)), max_frames, _ptr(n_frames), _ptr(marker_errors), _ptr(carry_out), _ptr(carry_bits_out), self._stream()))
        return frames, n_frames, marker_errors, carry_out, carry_bits_out

    def _rs_code(self, code):
        """the vit_hip_rs_code of an RSCode: made at its first use, kept as long as this decoder"""
        if code not in self._rs_codes:
            self._rs_codes[code] = _RsCode(self._handle, code)
        return self._rs_codes[code]

    def rs_decode(self, code, frames, n_frames=None, interleave: int = 1, out=None, status=None):
        """Reed-Solomon decoding (vit_hip_rs_decode_batch) of `frames`, the uint8 CUDA tensor [rows][max_frames][>= n * interleave]
        frames_extract returns (or [max_frames][...]: one row; the last stride is the frame stride): `code` is a reed_solomon.RSCode,
        symbol i of codeword c is frame byte i * interleave + c.  n_frames: the int32 CUDA tensor [rows] frames_extract returns -- frames
        at or behind it are neither read nor written, and neither is their status -- or None: all of them.  out: None decodes in place,
        or a tensor of the same shape and strides that does not overlap `frames`.  returns (frames, status): the tensor written and
        int32 [rows][max_frames][interleave], the byte errors corrected in each codeword or -1 where more than t = nroots // 2 stand in
        it (that codeword is left as received).  status = an int32 tensor of that size reuses it.  Nothing is copied to the host."""
        t = self.torch
        I = int(interleave)
        if I < 1:
            raise ValueError("interleave must be at least 1")
        rows, max_frames, stride = _args.packets(frames, "frames", code.n * I)
        out = frames if out is None else out
        if out is not frames and (_args.device(out, t.uint8, "out").shape != frames.shape or out.stride() != frames.stride()):
            raise ValueError("out must have the shape and strides of frames")
        _args.counts(n_frames, rows, "n_frames")
        if status is None:
            status = self._empty(tuple(frames.shape[:-1]) + (I,), t.int32)
        else:
            _args.dense(status, t.int32, rows * max_frames * I, "status")
        _lib.check(_lib.load().vit_hip_rs_decode_batch(self._handle._h, self._rs_code(code)._c, _ptr(frames), _ptr(out), stride, rows, max_frames,
                                                       _ptr(n_frames), I, _ptr(status), self._stream()))
        return out, status

    def deinterleave(self, packets, n_frames=None, branches: int = 12, cell: int = 17, hist=None, fill=None, packet_bytes: int = None,
                     out=None):
        """the convolutional (Forney) de-interleaver (vit_hip_deinterleave_batch; dvb.DVB_INTERLEAVER = (12, 17)) on `packets`, the
        uint8 CUDA tensor [rows][max_frames][>= n] frames_extract returns (or [max_frames][...]: one row; n = packet_bytes, by default
        the last dimension, a multiple of branches).  n_frames: the int32 CUDA tensor [rows] frames_extract returns, or None: all.
        hist / fill: the uint8 [rows][H n] and int32 [rows] the previous call returned as hist_out / fill_out (None: nothing carried), H
        = ceil((branches-1) cell branches / n).  returns (out, n_out, hist_out, fill_out): uint8 of the shape of `packets` of which the
        first n_out[r] (int32 [rows]) packets of row r are written -- byte i of packet k is stream byte (H + k) n + i - (branches-1 - i
        mod branches) cell branches of the real history packets followed by the input --, as rs_decode(interleave=1) takes them, and the
        last min(H, all) packets of that stream with their number.  out = the same four reuses those tensors; hist and hist_out must be
        distinct and have the same row stride.  Nothing is copied to the host."""
        t = self.torch
        B, M = int(branches), int(cell)
        n = int(packets.shape[-1]) if packet_bytes is None else int(packet_bytes)
        rows, mf, stride = _args.packets(packets, "packets", n)
        if B < 2 or M < 1 or n < 1 or n % B:
            raise ValueError("branches must be at least 2, cell at least 1, packet_bytes a multiple of branches")
        H = -(-(B - 1) * M * B // n)
        if out is None:
            out = (self._empty(tuple(packets.shape[:-1]) + (n,), t.uint8), self._empty(rows, t.int32), self._empty((rows, H * n), t.uint8),
                   self._empty(rows, t.int32))
        d_out, n_out, hist_out, fill_out = out
        orows, omf, ostride = _args.packets(d_out, "out[0]", n)
        if (orows, omf) != (rows, mf):
            raise ValueError(f"out[0] must hold [{rows}][{mf}] packets")
        _args.counts(n_frames, rows, "n_frames"), _args.counts(n_out, rows, "out[1]"), _args.counts(fill_out, rows, "out[3]")
        hstride = _args.carried(hist, fill, hist_out, rows, H * n, "hist", "fill")
        _lib.check(_lib.load().vit_hip_deinterleave_batch(
            self._handle._h, _ptr(packets), stride, rows, mf, _ptr(n_frames), B, M, n, _ptr(hist), _ptr(fill) if hist is not None else None,
            hstride, _ptr(d_out), ostride, _ptr(n_out), _ptr(hist_out), _ptr(fill_out), self._stream()))
        return d_out, n_out, hist_out, fill_out

    def dvb_derandomize(self, packets, n_frames=None, phase=None, rs_status=None, out=None, phase_out=None, sync_errors=None,
                        in_place: bool = False):
        """DVB-S energy-dispersal removal (vit_hip_dvb_derandomize_batch) on `packets`, uint8 CUDA [rows][max_frames][>= 188] (or
        [max_frames][...]: one row), of which the first 188 bytes of each are read -- 204-byte packets as rs_decode left them are fine.
        n_frames: int32 CUDA [rows] or None: all.  phase: int32 CUDA [rows], the place 0 .. 7 of packet 0 in its group of eight; a
        value outside (-1, say) or None means unknown: voted from this call's sync bytes.  rs_status: the int32 [rows][max_frames][1]
        rs_decode returned, or None: where negative, the packet's transport_error_indicator is set.  returns (out, phase_out,
        sync_errors): uint8 [rows][max_frames][188] of which the packets below n_frames are written -- byte 0 de-inverted at the head of
        a group, bytes 1 .. 187 XORed with dvb.dvb_prbs() --, int32 [rows] = the phase of the next call's packet 0 (-1 while unknown: a
        row without packets), int32 [rows][max_frames] = the bits the sync byte differs in from 0x47 (0xB8 at the head of a group).
        out / phase_out / sync_errors reuse tensors; in_place=True writes into `packets` (one workgroup per row: slower on long rows).
        Nothing is copied to the host."""
        t = self.torch
        rows, mf, stride = _args.packets(packets, "packets", 188)
        if in_place:
            if out is not None:
                raise ValueError("in_place=True writes into packets: no out")
            d_out, ostride = packets, stride
        else:
            d_out = self._empty(tuple(packets.shape[:-1]) + (188,), t.uint8) if out is None else out
            orows, omf, ostride = _args.packets(d_out, "out", 188)
            if (orows, omf) != (rows, mf):
                raise ValueError(f"out must hold [{rows}][{mf}] packets")
        _args.counts(n_frames, rows, "n_frames"), _args.counts(phase, rows, "phase")
        phase_out = self._empty(rows, t.int32) if phase_out is None else _args.counts(phase_out, rows, "phase_out")
        if sync_errors is None:
            sync_errors = self._empty(tuple(packets.shape[:-1]), t.int32)
        for x, what in ((sync_errors, "sync_errors"), (rs_status, "rs_status")):
            if x is not None:
                _args.dense(x, t.int32, rows * mf, what)
        _lib.check(_lib.load().vit_hip_dvb_derandomize_batch(
            self._handle._h, _ptr(packets), stride, int(packets.shape[-1]), rows, mf, _ptr(n_frames), _ptr(phase), _ptr(rs_status), _ptr(d_out),
            ostride, _ptr(phase_out), _ptr(sync_errors), self._stream()))
        return d_out, phase_out, sync_errors

    def crc_check(self, code, frames, n_bits: int, first_bit: int = 0, n_frames=None, field: bool = True, crc_out=None, syndrome_out=None):
        """the frame check (vit_hip_crc_batch): the CRC `code` (a crc.CRCCode: CCSDS_CRC16, LTE_CRC16, DAB_CRC16, LTE_CRC24A, ...) of bits
        [first_bit, first_bit + n_bits) of every frame of `frames`, uint8 CUDA [rows][max_frames][stride] (or [max_frames][stride]: one
        row; the bytes decode_tail_biting returns, the frames frames_extract and rs_decode wrote), bit t of a frame being bit 7 - t%8 of
        byte t/8.  n_frames: int32 CUDA [rows], frames at or behind it are neither read nor written and neither are their entries, or
        None: all.  field=True: the code.width bits behind the data are the transmitted field and the call returns (crc, syndrome),
        syndrome = crc ^ field: 0 where the frame checks, the RNTI on PDCCH, the antenna mask on PBCH; a frame must hold first_bit +
        n_bits + width bits.  field=False: returns crc alone, and a frame need only hold the data.  Both are int32 CUDA tensors of the
        shape frames.shape[:-1] that hold the uint32 values of the ABI (a width-32 value with its top bit set reads negative:
        .view(torch.uint32), or & 0xFFFFFFFF on an int64 copy); crc_out / syndrome_out reuse such tensors.  Nothing is copied to the
        host."""
        t = self.torch
        n_bits, first_bit = int(n_bits), int(first_bit)
        if n_bits < 0 or first_bit < 0:
            raise ValueError("n_bits and first_bit must not be negative")
        if syndrome_out is not None and not field:
            raise ValueError("syndrome_out needs field=True")
        rows, mf, stride = _args.packets(frames, "frames", (first_bit + n_bits + (code.width if field else 0) + 7) // 8)
        _args.counts(n_frames, rows, "n_frames")
        shape = tuple(frames.shape[:-1])
        crc = self._empty(shape, t.int32) if crc_out is None else _args.dense(crc_out, t.int32, rows * mf, "crc_out")
        syndrome = None
        if field:
            syndrome = self._empty(shape, t.int32) if syndrome_out is None else _args.dense(syndrome_out, t.int32, rows * mf, "syndrome_out")
        params = _lib.VitHipCrcParams(code.width, code.poly, code.init, code.xorout)
        at = _ptr(frames)
        if frames.numel() == 0 and rows * mf:                      # frames of no bytes (n_bits = 0, field=False): where they would start
            at = C.c_void_p(frames.untyped_storage().data_ptr() + frames.storage_offset())
        _lib.check(_lib.load().vit_hip_crc_batch(self._handle._h, C.byref(params), at, stride, rows, mf, _ptr(n_frames), first_bit,
                                                 n_bits, _ptr(crc), _ptr(syndrome), self._stream()))
        return (crc, syndrome) if field else crc

    def dab_descramble(self, frames, n_bits: int, n_frames=None, out=None, in_place: bool = False):
        """DAB energy-dispersal removal (vit_hip_dab_descramble_batch; ETSI EN 300 401 clause 10) on `frames`, the uint8 CUDA tensor
        [rows][max_frames][>= ceil(n_bits/8)] (or [max_frames][...]: one row) decode returns: bit t < n_bits of every frame, bit t being
        bit 7 - t%8 of byte t/8, is XORed with the sequence of x^9 + x^5 + 1 from its start (dab.dab_prbs); the bits at or behind n_bits
        in the last byte are copied unchanged.  n_frames: int32 CUDA [rows], frames at or behind it are neither read nor written, or
        None: all.  returns uint8 [rows][max_frames][ceil(n_bits/8)]; out reuses a tensor (its last stride is the frame stride);
        in_place=True writes into `frames`.  Dispersal is its own inverse.  Nothing is copied to the host."""
        t = self.torch
        n_bits = int(n_bits)
        if n_bits < 0:
            raise ValueError("n_bits must not be negative")
        nb = (n_bits + 7) // 8
        rows, mf, stride = _args.packets(frames, "frames", nb)
        if in_place:
            if out is not None:
                raise ValueError("in_place=True writes into frames: no out")
            d_out, ostride = frames, stride
        else:
            d_out = self._empty(tuple(frames.shape[:-1]) + (nb,), t.uint8) if out is None else out
            orows, omf, ostride = _args.packets(d_out, "out", nb)
            if (orows, omf) != (rows, mf):
                raise ValueError(f"out must hold [{rows}][{mf}] frames")
        _args.counts(n_frames, rows, "n_frames")
        if rows * mf == 0 or nb == 0:
            return d_out
        _lib.check(_lib.load().vit_hip_dab_descramble_batch(self._handle._h, _ptr(frames), stride, rows, mf, _ptr(n_frames), n_bits,
                                                            _ptr(d_out), ostride, self._stream()))
        return d_out

    def dabplus_sync(self, frames, frame_bytes: int = None, n_frames=None, frame0: int = 0, out=None, accumulate=False):
        """DAB+ superframe synchronisation (vit_hip_dabplus_sync; ETSI TS 102 563) on `frames`, the uint8 CUDA tensor
        [rows][max_frames][>= frame_bytes] of logical frames DabSubchannelDecoder.push returns (or [max_frames][...]: one row; any view
        whose frames are contiguous and evenly spaced; frame_bytes = 24 s defaults to the last dimension and is at least 11): frame f
        hits where its bytes 0 .. 1 are the Fire code (dabplus.FIRECODE) of bytes 2 .. 10 and the eleven are not all zero, and counts
        for phase (frame0 + f) mod 5.  n_frames: int32 CUDA [rows] or None: all.  returns (hits, count, lock): int32 CUDA [rows][5],
        [rows][5] and [rows][4] = (phase, inverted, errors, compared), the phase in bits as frames_extract reads it at period = 40 *
        frame_bytes with phase0 = frame0 * 8 * frame_bytes; errors == compared means no frame has hit.  out = (hits, count, lock) reuses
        those tensors; with accumulate=True the call adds to the totals they hold and the lock is that of the totals.  Nothing is copied
        to the host."""
        t = self.torch
        fb = int(frames.shape[-1]) if frame_bytes is None else int(frame_bytes)
        rows, mf, rs, fs = _args.dabplus_frames(frames, fb, int(frame0))
        _args.counts(n_frames, rows, "n_frames")
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True adds to the totals of out=(hits, count, lock)")
            out = (self._empty((rows, 5), t.int32), self._empty((rows, 5), t.int32), self._empty((rows, 4), t.int32))
        hits, count, lock = out
        for x, n, what in ((hits, 5, "out[0]"), (count, 5, "out[1]"), (lock, 4, "out[2]")):
            _args.dense(x, t.int32, rows * n, what)
        _lib.check(_lib.load().vit_hip_dabplus_sync(self._handle._h, _ptr(frames), rs, fs, fb, rows, mf, _ptr(n_frames), int(frame0),
                                                    _lib.MARKER_ACCUMULATE if accumulate else 0, _ptr(hits), _ptr(count), _ptr(lock),
                                                    self._stream()))
        return hits, count, lock

    def dabplus_au_table(self, superframes, s: int, n_frames=None, rs_status=None, out=None):
        """the access-unit table of DAB+ audio superframes (vit_hip_dabplus_au_batch) on `superframes`, the uint8 CUDA tensor
        [rows][max_frames][>= 110 s] frames_extract wrote at period 960 s and rs_decode(dabplus.DABPLUS_RS_120_110, interleave=s)
        corrected (or [max_frames][...]: one row; the last stride is the frame stride).  n_frames: int32 CUDA [rows], superframes at
        or behind it are neither read nor written and neither are their entries, or None: all.  rs_status: the int32
        [rows][max_frames][s] rs_decode returned, or None.  returns (info, au): int32 CUDA [rows][max_frames] = fire_ok | consistent <<
        1 | rs_failed << 2 | n_aus << 4 | byte2 << 8 (n_aus 0 unless the superframe is valid) and int32 [rows][max_frames][6][3] =
        (start, bytes, syndrome) per access unit: syndrome 0 where its CRC-16 checks, (0, 0, -1) for a slot without one.  Both hold the
        uint32 values of the ABI.  out = (info, au) reuses those tensors.  Nothing is copied to the host."""
        t = self.torch
        s = int(s)
        if not 1 <= s <= 24:
            raise ValueError("s must be 1 .. 24")
        rows, mf, stride = _args.packets(superframes, "superframes", 110 * s)
        _args.counts(n_frames, rows, "n_frames")
        if rs_status is not None:
            _args.dense(rs_status, t.int32, rows * mf * s, "rs_status")
        shape = tuple(superframes.shape[:-1])
        if out is None:
            out = (self._empty(shape, t.int32), self._empty(shape + (6, 3), t.int32))
        info, au = out
        _args.dense(info, t.int32, rows * mf, "out[0]"), _args.dense(au, t.int32, rows * mf * 18, "out[1]")
        if rows * mf == 0:
            return info, au
        _lib.check(_lib.load().vit_hip_dabplus_au_batch(self._handle._h, _ptr(superframes), stride, rows, mf, _ptr(n_frames), s,
                                                        _ptr(rs_status), _ptr(info), _ptr(au), self._stream()))
        return info, au
