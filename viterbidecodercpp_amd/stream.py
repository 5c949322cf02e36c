"""The chunked receivers on top of BatchDecoder.decode_streams: push() symbols as they arrive, get decoded bytes back.

`MultiStreamDecoder` serves n lockstep streams and holds what there is to chunking: the hold-back rule, the log of internal calls, the
sub-byte carry, the running channel error and marker totals and the first / done state.  What happens to the emitted bits behind the
marker search -- frames, de-interleaver, Reed-Solomon, derandomiser -- is one `_FrameChain`.  `StreamDecoder` is the n_streams = 1 face
(vit_hip_decode_streams with one stream launches exactly what vit_hip_decode_stream launches).
"""
from __future__ import annotations

import numpy as np

from . import _args
from .decoder import BatchDecoder


def _next_states(states, bits, K):
    """decoder states [n] after the input bits [n][n_bits] (0/1) have been shifted in: bit j = the input bit j+1 steps back"""
    states = np.asarray(states, dtype=np.int64).copy()
    for j in range(max(bits.shape[1] - (K - 1), 0), bits.shape[1]):
        states = (states << 1) | bits[:, j].astype(np.int64)
    return states & ((1 << (K - 1)) - 1)


class _FrameChain:
    """What a receiver does on the device with the bits of an internal call behind the marker search: extract -> [de-interleave] ->
    [Reed-Solomon] -> [derandomise], with the state each stage carries from call to call in two buffers it reads and writes in turn, and
    the frames that came out, per stream, until take() hands them over.  `branches` and `cell` are None without de-interleaver, `rs` is
    None without Reed-Solomon code; `packet_bytes` = period / 8 is the de-interleaver's packet."""

    def __init__(self, decoder, n_streams, frames, marker, marker_bits, period, drop_bits, pad, rs, rs_interleave, deinterleave, derandomize):
        if not frames or marker is None or not 8 <= int(period) or not 0 <= int(drop_bits) < int(period) or marker_bits > int(period):
            raise ValueError("frames=True (rs=, deinterleave= and dvb_derandomize= need it) needs marker=(value, bits), period=P >= max(8, bits) "
                             "and 0 <= frame_drop_bits < P")
        t, n, P = decoder.torch, n_streams, int(period)
        self.decoder, self.n_streams, self.marker, self.marker_bits, self.period, self.drop_bits = decoder, n, marker, marker_bits, P, int(drop_bits)
        self.frame_bytes = (P - self.drop_bits + 7) // 8
        self.pad = None
        if pad is not None:
            pad = pad if t.is_tensor(pad) else t.from_numpy(np.frombuffer(bytes(pad), dtype=np.uint8).copy())
            self.pad = pad.to(device=decoder.device, dtype=t.uint8).reshape(-1).contiguous()
            if self.pad.numel() < self.frame_bytes:
                raise ValueError(f"frame_pad must hold ceil((period - frame_drop_bits) / 8) = {self.frame_bytes} bytes")
        self.rs, self.rs_interleave = rs, int(rs_interleave)
        if rs is not None and (self.rs_interleave < 1 or P - self.drop_bits != 8 * rs.n * self.rs_interleave):
            raise ValueError("rs= needs frames=True and (period - frame_drop_bits) / 8 == rs.n * rs_interleave")
        self.branches = self.cell = None
        self.derandomize, self.packet_bytes = bool(derandomize), P // 8
        zeros = lambda *shape: t.zeros(shape, dtype=t.int32, device=decoder.device)                   # noqa: E731
        if deinterleave is not None:
            B, M, nb = int(deinterleave[0]), int(deinterleave[1]), self.packet_bytes
            if self.drop_bits or pad is not None or P % 8 or B < 2 or M < 1 or nb % B or (rs is not None and self.rs_interleave != 1):
                raise ValueError("deinterleave=(B, M) needs frames=True, frame_drop_bits=0, no frame_pad, period = 8 n with n a multiple of B, "
                                 "and with rs= rs_interleave=1 and rs.n == n")
            H = -(-(B - 1) * M * B // nb)
            if (H + 1) * nb > 32768:
                raise ValueError("deinterleave=(B, M): (H + 1) * n is above 32768 (vit_hip_deinterleave_batch)")
            if derandomize and nb < 188:
                raise ValueError("dvb_derandomize=True needs packets of at least 188 bytes")
            self.branches, self.cell = B, M
            # history, fill and group phase of every stream: a call reads one triple and writes the other
            self.delay, self.delay_next = ((t.zeros((n, H * nb), dtype=t.uint8, device=decoder.device), zeros(n), zeros(n) - 1) for _ in range(2))
            self.lock = zeros(n, 2)                                   # the (phase, inverted) the last extraction cut at
        elif derandomize:
            raise ValueError("dvb_derandomize=True needs deinterleave=(B, M)")
        # the unfinished frame of every stream and its bits: a call reads one pair and writes the other
        self.carry, self.carry_next = ((t.zeros((n, (P + 6) // 8), dtype=t.uint8, device=decoder.device), zeros(n)) for _ in range(2))
        self.done = [[] for _ in range(n)]                            # (frames, marker_errors[, rs_status][, crc_syndrome]) per call, until taken
        self.crc = None                                               # (CRCCode, n_bits, first_bit) once frame_crc() has asked for the check

    def check_crc(self, code, n_bits, first_bit):
        """MultiStreamDecoder.frame_crc: the frame check behind rs_decode (behind the extraction without rs=) from the next call on"""
        n_bits, first_bit = int(n_bits), int(first_bit)
        if self.branches is not None or self.derandomize:
            raise ValueError("frame_crc: transport packets (deinterleave=, dvb_derandomize=) carry no frame CRC")
        if n_bits < 0 or first_bit < 0 or first_bit + n_bits + code.width > self.period - self.drop_bits:
            raise ValueError(f"frame_crc: first_bit + n_bits + width exceeds the {self.period - self.drop_bits} bits of a frame")
        self.crc = (code, n_bits, first_bit)

    def run(self, out, n_bits, phase0, lock):
        """out [n_streams][ceil(n_bits/8)]: the bits the call emitted, bit 0 at phase phase0; lock [n_streams][4]: that of the totals so far"""
        t, dec = self.decoder.torch, self.decoder
        cap = dec.frames_capacity(n_bits, self.period)
        fresh = (t.empty((self.n_streams, cap, self.frame_bytes), dtype=t.uint8, device=dec.device),
                 t.empty(self.n_streams, dtype=t.int32, device=dec.device), t.empty((self.n_streams, cap), dtype=t.int32, device=dec.device))
        carry, carry_bits = self.carry
        frames, n, errors, _, _ = dec.frames_extract(out, n_bits, self.period, phase0, lock, carry, carry_bits, self.marker, self.marker_bits,
                                                     self.drop_bits, self.pad, out=fresh + self.carry_next)
        self.carry, self.carry_next = self.carry_next, self.carry
        status, n_errors = None, n                                # `errors` holds one entry per frame extracted ...
        if self.branches is not None:
            frames, n, errors, status = self._dvb(frames, n, errors, lock[:, :2])
            if self.derandomize:
                n_errors = n                                      # ... or, derandomised, one per packet that came out
        elif self.rs is not None and frames.shape[1]:
            _, status = dec.rs_decode(self.rs, frames, n, self.rs_interleave)
        syndrome = None
        if self.crc is not None:
            syndrome = t.zeros(tuple(frames.shape[:2]), dtype=t.int32, device=dec.device)
            if frames.shape[1]:
                dec.crc_check(self.crc[0], frames, self.crc[1], self.crc[2], n, syndrome_out=syndrome)
            syndrome = syndrome.cpu().numpy().view(np.uint32).astype(np.int64)
        status = None if status is None else status.cpu().numpy()
        n_errors = n_errors.cpu().numpy()
        n, frames, errors = n.cpu().numpy(), frames.cpu().numpy(), errors.cpu().numpy().view(np.uint32).astype(np.int64)
        for i in range(self.n_streams):
            if n[i] or n_errors[i]:
                done = (frames[i, :n[i]].copy(), errors[i, :n_errors[i]].copy())
                done = done if status is None else done + (status[i, :n[i]].copy(),)
                self.done[i].append(done if syndrome is None else done + (syndrome[i, :n[i]].copy(),))

    def _dvb(self, frames, n, errors, lock):
        """the packets one extraction wrote at `lock` [n_streams][2] -> de-interleaved, Reed-Solomon decoded in place, derandomised:
        (packets, their number per stream, sync_errors -- or the marker_errors as they came --, rs_status or None), all on the device"""
        t, dec = self.decoder.torch, self.decoder
        changed = (lock != self.lock).any(dim=1)
        self.lock = lock.clone()
        hist, fill, phase = self.delay
        hist_out, fill_out, phase_out = self.delay_next
        self.delay, self.delay_next = self.delay_next, self.delay
        fill = t.where(changed, t.zeros_like(fill), fill)
        phase = t.where(changed, t.full_like(phase, -1), phase)
        out, n_out, _, _ = dec.deinterleave(frames, n, self.branches, self.cell, hist, fill,
                                            out=(t.empty_like(frames), t.empty(self.n_streams, dtype=t.int32, device=dec.device), hist_out, fill_out))
        status = None
        if self.rs is not None:
            _, status = dec.rs_decode(self.rs, out, n_out, 1)
        if self.derandomize:
            out, _, errors = dec.dvb_derandomize(out, n_out, phase, status, phase_out=phase_out)
        return out, n_out, errors, status

    def take(self):
        """per stream what came out since the last take, in order; see MultiStreamDecoder.take_frames"""
        empty = (np.zeros((0, 188 if self.derandomize else self.frame_bytes), dtype=np.uint8), np.zeros(0, dtype=np.int64))
        if self.rs is not None:
            empty += (np.zeros((0, self.rs_interleave), dtype=np.int32),)
        if self.crc is not None:
            empty += (np.zeros(0, dtype=np.int64),)
        taken = [tuple(np.concatenate(part) for part in zip(*done)) if done else empty for done in self.done]
        self.done = [[] for _ in range(self.n_streams)]
        return taken


class MultiStreamDecoder:
    """A chunked receiver for n_streams lockstep streams: push() the same number of steps of each stream as they arrive, get one
    `bytes` per stream back; finish() ends all streams (their last K-1 steps are the zero tail).

    The pending symbols of all streams live in ONE device buffer [n_streams][pitch][R] whose pitch is rounded up to a multiple of
    the window (and grown when a push needs it), so every internal call reads them in place on one shared window grid.

    Every internal call is a segment of head + n*window + tail steps on the window grid (one uniform batch), BEGIN on the first.
    What does not fill a window yet stays on the device: the last head + tail steps of the segment just decoded (the next one's
    lead-in and this one's look-ahead) and at least one more window (window + K-1 steps), so that the final segment under END
    always holds a full window -- with that, pushes of ANY sizes plus finish() decode, per stream, to exactly the bits of ONE
    decode_stream call over that whole stream (tests/test_stream_cpu.py: chunked vs one call).  Whole bytes only: the sub-byte
    remainder is carried to the next call; finish() pads the last byte with zeros.  `n_bits` counts the bits returned so far per
    stream.

    channel_errors=True: the object also keeps `.channel_errors`, two int64 arrays of length n_streams: the running (errors,
    compared) of the re-encoded channel symbol error count (BatchDecoder.channel_errors) over every trellis step whose bit has been
    emitted so far -- each step exactly once, however the pushes were cut; finish() adds the K-1 tail steps.  One more launch and
    one small read-back per internal call for all streams; the last K-1 emitted bits are carried as the next call's start state.
    Off (the default), nothing changes.

    marker=(value, bits) with period=P (frame_sync.CCSDS_ASM, DVB_SYNC): the object also keeps the running per-phase totals of the
    frame marker search (BatchDecoder.marker_search) over everything it emits: `.marker_totals` = (distance, count), int64 arrays
    [n_streams][P], and `.marker_lock`, per stream the (phase, inverted, errors, compared) those totals name.  Every marker position
    of the whole emitted stream is counted exactly once, however the pushes were cut -- the last bits-1 emitted bits are carried as
    the next call's history --, and a phase is counted from the stream's first emitted bit.  One more accumulate-mode search per
    internal call; the totals live on the device as 32-bit counters (they wrap past 2^32 - 1).  Off (the default), nothing changes.

    frames=True (needs marker and period >= 8): after the search of every internal call the object cuts the emitted bits into frames
    on the device (BatchDecoder.frames_extract) at the lock as it stands after that call: each frame from bit 0 of a byte on,
    complemented under an inverted lock, without its first frame_drop_bits bits (the marker, say), XORed with frame_pad (uint8,
    ceil(Q/8) bytes for the Q = P - frame_drop_bits output bits: frame_sync.ccsds_randomizer).  The unfinished frame at the end of a
    call stays on the device in one of two carry buffers and is completed by a later call, however the pushes were cut.
    take_frames() returns, per stream, (uint8 [n][ceil(Q/8)], marker_errors int64 [n]) for the frames completed since the last
    take; whether to trust a frame is the caller's decision, from its marker_errors.  Off (the default), nothing changes.

    rs=RSCode, rs_interleave=I (needs frames=True and (P - frame_drop_bits) / 8 == n * I): right behind every extraction the frames are
    Reed-Solomon decoded in place on the device (BatchDecoder.rs_decode), and take_frames() returns (frames, marker_errors,
    rs_status), rs_status int32 [n][I]: the byte errors corrected in each codeword, or -1 where it was left as received.  Without rs=
    nothing changes, the 2-tuple included.

    deinterleave=(B, M) (dvb.DVB_INTERLEAVER; needs frames=True, frame_drop_bits=0, no frame_pad and P = 8 n with n a multiple of B; with
    rs= also rs_interleave=1 and rs.n == n): the frames are the n-byte packets of a convolutionally interleaved stream, the sync byte in
    front.  Every internal call runs extract -> BatchDecoder.deinterleave -> rs_decode in place -> (dvb_derandomize=True, n >= 188:)
    BatchDecoder.dvb_derandomize on the device; the de-interleaver's history and fill and the group phase stay there in ping-ponged
    buffers.  When a stream's (phase, inverted) lock differs from the one the call before extracted at, its fill and group phase are
    reset on the device (a torch.where on the lock tensors: no read-back), so the packets of the old alignment never meet those of the
    new one; the first H = ceil((B-1) M B / n) packets behind every (re-)lock fill the delay lines and give no output.  take_frames()
    then returns per stream (packets, errors[, rs_status]) -- see there.  Without the two keywords nothing changes."""

    # how the errors word it; StreamDecoder has its own
    _RULE = "n_streams, window, head, tail outside the argument rule of vit_hip_decode_streams"
    _SHAPE, _FINISHED, _EMPTY = "[n_streams][steps][R]", "the streams are finished", "empty streams"

    def __init__(self, decoder: BatchDecoder, n_streams: int, window: int = None, head: int = None, tail: int = None,
                 channel_errors: bool = False, marker=None, period: int = None, frames: bool = False, frame_drop_bits: int = 0,
                 frame_pad=None, rs=None, rs_interleave: int = 1, deinterleave=None, dvb_derandomize: bool = False):
        self.decoder = decoder
        self.n_streams = n = int(n_streams)
        self.window, self.head, self.tail, _ = decoder._stream_args(window, head, tail, True, False)
        seg = self.head + self.window + self.tail
        pitch = -(-seg // self.window) * self.window
        if n < 1 or decoder.streams_workspace_bytes(n, pitch, seg, True, False, self.window, self.head, self.tail) == 0:
            raise ValueError(self._RULE)
        self.n_bits = 0
        self.calls = []                       # (steps, begin, end) of every internal call, for inspection
        self._first = True
        self._done = False
        self._buf = None                      # device tensor [n_streams][pitch][R], pitch % window == 0
        self._pending = 0                     # steps of it in use, per stream
        self._carry = np.zeros((n, 0), dtype=np.uint8)
        self._errors = self._compared = None  # the channel error totals per stream, when they are kept
        if channel_errors:
            self._errors, self._compared = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
            self._state = np.zeros(n, dtype=np.int64)                 # the last K-1 emitted bits, as a decoder state
        self._marker = self._marker_bits = self._period = None
        if marker is not None:
            value, bits = int(marker[0]), int(marker[1])
            if period is None or not 1 <= int(period) < 1 << 31 or not 1 <= bits <= 64 or value >> bits:
                raise ValueError("marker=(value, bits) needs 1 <= bits <= 64, no bit of value above them, and period=P >= 1")
            t = decoder.torch
            self._marker, self._marker_bits, self._period = value, bits, int(period)
            # the running totals per phase and the lock they name, on the device
            self._distance, self._count = (t.zeros((n, int(period)), dtype=t.int32, device=decoder.device) for _ in range(2))
            self._lock = t.zeros((n, 4), dtype=t.int32, device=decoder.device)
            self._emitted = 0                                         # bits the internal calls have emitted, per stream
            self._recent = np.zeros((n, 0), dtype=np.uint8)           # the last bits-1 of them
        self._chain = None
        if frames or rs is not None or deinterleave is not None or dvb_derandomize:
            self._chain = _FrameChain(decoder, n, frames, self._marker, self._marker_bits, period, frame_drop_bits, frame_pad, rs, rs_interleave,
                                      deinterleave, dvb_derandomize)

    @property
    def channel_errors(self):
        if self._errors is None:
            raise AttributeError("this receiver was made without channel_errors=True")
        return self._errors, self._compared

    def _count(self, out, bits, n_bits, end):
        """out [n_streams][ceil(n_bits/8)]: the bits the call emitted (`bits`, unpacked), from the segment's first emitted step on"""
        dec = self.decoder
        err, cmp = dec.channel_errors(self._buf[:, 0 if self._first else self.head:], out, n_bits, tail=end, start_state=self._state,
                                      symbol_frame_stride=self._buf.shape[1] * dec.R)
        self._errors, self._compared = self._errors + err.cpu().numpy(), self._compared + cmp.cpu().numpy()
        self._state = _next_states(self._state, bits, dec.K)

    def _no_marker(self):
        if self._marker is None:
            raise AttributeError("this receiver was made without marker=(value, bits) and period=P")

    @property
    def marker_totals(self):
        self._no_marker()
        return tuple(x.cpu().numpy().view(np.uint32).astype(np.int64) for x in (self._distance, self._count))

    @property
    def marker_lock(self):
        self._no_marker()
        return [tuple(int(v) for v in row) for row in self._lock.cpu().numpy().view(np.uint32)]

    def _search(self, out, bits, n_bits):
        """out [n_streams][ceil(n_bits/8)]: the bits the call emitted (`bits`, unpacked); the history is what was emitted before them"""
        m, P = self._marker_bits, self._period
        hb = self._recent.shape[1]
        if n_bits + hb >= m:
            history = [int("".join(map(str, row)), 2) if hb else 0 for row in self._recent]
            self.decoder.marker_search(out, n_bits, self._marker, m, P, self._emitted % P, history, hb,
                                       out=(self._distance, self._count, self._lock), accumulate=True)
        bits = np.concatenate([self._recent, bits], axis=1)
        self._recent = bits[:, max(bits.shape[1] - (m - 1), 0):]
        self._emitted += n_bits

    def take_frames(self) -> list:
        """per stream (frames uint8 [n][ceil(Q/8)], marker_errors int64 [n]) -- with rs= also rs_status int32 [n][I] --: the frames
        completed since the last take, in order.
        With deinterleave=(B, M) the first element holds the de-interleaved packets, uint8 [k][P/8]: packet k of a take is packet k of
        the rule of vit_hip_deinterleave_batch over the packets extracted since the last (re-)lock, Reed-Solomon corrected with rs=.  The
        second element is then still the marker_errors of the frames EXTRACTED since the last take, one per input packet, int64 [m] with m
        >= k (the packets that fill the delay lines are counted too).  With dvb_derandomize=True the first element is the transport
        packets, uint8 [k][188], by the rule of vit_hip_dvb_derandomize_batch, and the second their sync_errors, int64 [k]: the bits the
        sync byte differed in from 0x47, or from 0xB8 at the head of a group of eight.  rs_status, int32 [k][1], is there exactly with
        rs=.  After frame_crc() one further, last element: crc_syndrome int64 [n] (see there)."""
        if self._chain is None:
            raise AttributeError("this receiver was made without frames=True")
        return self._chain.take()

    def frame_crc(self, code, n_bits: int, first_bit: int = 0):
        """the frame check on the device (BatchDecoder.crc_check), asked for before the first push: `code` is a crc.CRCCode
        (CCSDS_CRC16: the frame error control field), the data are bits [first_bit, first_bit + n_bits) of every frame as take_frames()
        returns it, the transmitted field the code.width bits behind them.  Every internal call then runs the check right behind
        rs_decode (corrected frames are checked; without rs= behind the extraction), and take_frames() returns one further, last element
        per stream: crc_syndrome int64 [n] = crc ^ field, 0 where the frame checks.  rs_status >= 0 says a codeword is valid, not that
        it is the one sent: this is what tells.  ValueError after a push, without frames=True, with deinterleave= or dvb_derandomize=
        (transport packets carry no frame CRC), and when first_bit + n_bits + width exceeds the frame."""
        if self.calls or self._buf is not None or self._done:
            raise ValueError("frame_crc must be called before the first push")
        if self._chain is None:
            raise ValueError("frame_crc needs frames=True")
        self._chain.check_crc(code, n_bits, first_bit)

    def _append(self, symbols):
        if symbols is None:
            return
        dec = self.decoder
        if _args.device(symbols, dec._soft_dtype, "symbols").dim() < 2 or symbols.shape[0] != self.n_streams or symbols[0].numel() % dec.R != 0:
            raise ValueError(f"symbols must be {self._SHAPE}")
        symbols = symbols.reshape(self.n_streams, -1, dec.R)
        P, n = self._pending, symbols.shape[1]
        if self._buf is None or P + n > self._buf.shape[1]:
            # room for what is held back between calls as well, so that a steady flow of pushes of this size does not grow it again
            pitch = -(-(P + n + self.head + 2 * self.window + self.tail) // self.window) * self.window
            buf = dec.torch.empty((self.n_streams, pitch, dec.R), dtype=dec._soft_dtype, device=dec.device)
            if P:
                buf[:, :P] = self._buf[:, :P]
            self._buf = buf
        self._buf[:, P:P + n] = symbols
        self._pending = P + n

    def _decode(self, steps, end):
        """one internal call over the first `steps` pending steps of every stream: the bytes it hands back, per stream"""
        out, n_bits = self.decoder.decode_streams(self._buf, steps, self._first, end, self.window, self.head, self.tail)
        self.calls.append((steps, self._first, end))
        bits = np.unpackbits(out.cpu().numpy(), axis=1)[:, :n_bits]       # the one read-back of the emitted bits
        if self._errors is not None:
            self._count(out, bits, n_bits, end)
        if self._marker is not None:
            phase0 = self._emitted % self._period
            self._search(out, bits, n_bits)
            if self._chain is not None and n_bits:
                self._chain.run(out, n_bits, phase0, self._lock)
        self._first = False
        # whole bytes only: the rest waits in the carry, which the last call flushes
        bits = np.concatenate([self._carry, bits], axis=1)
        keep = bits.shape[1] if end else bits.shape[1] - bits.shape[1] % 8
        self._carry = bits[:, keep:]
        self.n_bits += keep
        return [np.packbits(row[:keep], bitorder="big").tobytes() for row in bits]

    def push(self, symbols) -> list:
        if self._done:
            raise RuntimeError(self._FINISHED)
        self._append(symbols)
        P = self._pending
        hold = self.head + self.window + self.decoder.K - 1
        if P < hold + self.window:
            return [b""] * self.n_streams
        n = (P - hold) // self.window
        data = self._decode(self.head + n * self.window + self.tail, False)
        self._pending = P - n * self.window
        self._buf[:, :self._pending] = self._buf[:, n * self.window:P].clone()
        return data

    def finish(self, symbols=None) -> list:
        if self._done:
            raise RuntimeError(self._FINISHED)
        self._append(symbols)
        if self._buf is None:
            raise ValueError(self._EMPTY)
        data = self._decode(self._pending, True)
        self._done = True
        self._buf = None
        self._pending = 0
        return data


class StreamDecoder(MultiStreamDecoder):
    """MultiStreamDecoder for ONE long stream: push() and finish() take any tensor of whole trellis steps ([steps][R], flat, or a view
    that is not contiguous) and return `bytes`; `.channel_errors` (with channel_errors=True) is a pair of ints, `.marker_totals` (with
    marker and period) a pair of [P] arrays and `.marker_lock` one (phase, inverted, errors, compared); take_frames() (with
    frames=True) returns the one (frames, marker_errors) pair, or with rs= the one (frames, marker_errors, rs_status) triple; with
    deinterleave= / dvb_derandomize= what MultiStreamDecoder.take_frames says, for the one stream."""

    _RULE = "window, head, tail outside the argument rule of vit_hip_decode_stream"
    _SHAPE, _FINISHED, _EMPTY = "[steps][R]", "the stream is finished", "an empty stream"

    def __init__(self, decoder: BatchDecoder, window: int = None, head: int = None, tail: int = None, channel_errors: bool = False,
                 marker=None, period: int = None, frames: bool = False, frame_drop_bits: int = 0, frame_pad=None, rs=None,
                 rs_interleave: int = 1, deinterleave=None, dvb_derandomize: bool = False):
        super().__init__(decoder, 1, window=window, head=head, tail=tail, channel_errors=channel_errors, marker=marker, period=period,
                         frames=frames, frame_drop_bits=frame_drop_bits, frame_pad=frame_pad, rs=rs, rs_interleave=rs_interleave,
                         deinterleave=deinterleave, dvb_derandomize=dvb_derandomize)

    def take_frames(self):
        return super().take_frames()[0]

    @property
    def marker_totals(self):
        distance, count = super().marker_totals
        return distance[0], count[0]

    @property
    def marker_lock(self):
        return super().marker_lock[0]

    @property
    def channel_errors(self):
        errors, compared = super().channel_errors
        return int(errors[0]), int(compared[0])

    def push(self, symbols) -> bytes:
        return super().push(None if symbols is None else symbols[None])[0]

    def finish(self, symbols=None) -> bytes:
        return super().finish(None if symbols is None else symbols[None])[0]
