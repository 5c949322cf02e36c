"""DAB+ audio superframes (ETSI TS 102 563) behind the DAB receive chain: the codes, the rules of vit_hip_dabplus_sync and
vit_hip_dabplus_au_batch on the host (include/vit_hip.h), the transmit side, and DabPlusDecoder, the route from a sub-channel's soft bits
to checked access units on the device: DabSubchannelDecoder.push -> BatchDecoder.dabplus_sync -> frames_extract -> rs_decode ->
dabplus_au_table.  A sub-channel of index s = 1 .. 24 has logical frames of 24 s bytes; five of them are a superframe of 120 s bytes, the
first 110 s data, the rest the parity of s interleaved RS(120,110) codewords.  AAC decoding and PAD extraction are not here."""
from __future__ import annotations

import numpy as np

from .crc import DAB_CRC16, CRCCode, crc_numpy
from .dab import DabSubchannelDecoder
from .reed_solomon import RSCode, rs_encode_numpy

DABPLUS_RS_120_110 = RSCode(0x11D, 0, 1, 10, pad=135)              # the (255,245) code shortened by 135; symbol i of codeword c is byte i s + c
FIRECODE = CRCCode(16, 0x782F, 0, 0)                               # over bytes 2 .. 10 of a superframe, sent in bytes 0 .. 1
DABPLUS_FORMATS = {(0, 1): (2, 5), (1, 1): (3, 6), (0, 0): (4, 8), (1, 0): (6, 11)}   # (dac_rate, sbr_flag) -> (n_aus, au_start[0])


def firecode_hit_numpy(frames) -> np.ndarray:
    """frames uint8 [...][>= 11] -> bool [...]: the Fire code of bytes 2 .. 10 stands in bytes 0 .. 1, and the eleven are not all zero"""
    x = np.asarray(frames, dtype=np.uint8)
    if x.shape[-1] < 11:
        raise ValueError("a header has 11 bytes")
    field = x[..., 0].astype(np.int64) * 256 + x[..., 1]
    return (crc_numpy(FIRECODE, np.ascontiguousarray(x[..., 2:11]), 72) == field) & x[..., :11].any(axis=-1)


def dabplus_lock_numpy(hits, count, frame_bytes: int) -> np.ndarray:
    """the lock of vit_hip_dabplus_sync from per-phase totals [rows][5]: int64 [rows][4] of (phase in bits, 0, errors, compared)"""
    hits, count = np.atleast_2d(np.asarray(hits, dtype=np.int64)), np.atleast_2d(np.asarray(count, dtype=np.int64))
    out = np.zeros((hits.shape[0], 4), dtype=np.int64)
    for r in range(hits.shape[0]):
        best = (0, int(count[r, 0] - hits[r, 0]), int(count[r, 0]))
        for p in range(1, 5):
            e, c = int(count[r, p] - hits[r, p]), int(count[r, p])
            if c > 0 and (best[2] == 0 or e * best[2] < best[1] * c):
                best = (p, e, c)
        out[r] = (best[0] * 8 * int(frame_bytes), 0, best[1], best[2])
    return out


def dabplus_sync_numpy(frames, n_frames=None, frame0: int = 0, frame_bytes: int = None, totals=None):
    """the rule of vit_hip_dabplus_sync: frames uint8 [rows][F][>= 11] (or [F][...]: one row), n_frames [rows] or None, totals = (hits,
    count) to add to or None.  returns (hits, count, lock): int64 [rows][5], [rows][5], [rows][4]"""
    x = np.asarray(frames, dtype=np.uint8)
    x = x[None] if x.ndim == 2 else x
    rows, F = x.shape[:2]
    fb = int(x.shape[-1]) if frame_bytes is None else int(frame_bytes)
    if not 0 <= int(frame0) < 5 or fb < 11 or x.shape[-1] < 11:
        raise ValueError("outside the argument rule of vit_hip_dabplus_sync")
    hits = np.zeros((rows, 5), dtype=np.int64) if totals is None else np.array(totals[0], dtype=np.int64).reshape(rows, 5)
    count = np.zeros((rows, 5), dtype=np.int64) if totals is None else np.array(totals[1], dtype=np.int64).reshape(rows, 5)
    hit = firecode_hit_numpy(x) if F else np.zeros((rows, 0), dtype=bool)
    for r in range(rows):
        nf = F if n_frames is None else min(int(np.asarray(n_frames).reshape(-1)[r]) & 0xFFFFFFFF, F)
        for f in range(nf):
            p = (int(frame0) + f) % 5
            count[r, p] += 1
            hits[r, p] += int(hit[r, f])
    return hits, count, dabplus_lock_numpy(hits, count, fb)


def dabplus_header_numpy(superframe, s: int):
    """ONE superframe's header: (fire_ok, consistent, n_aus, au_start [n_aus + 1], byte2)"""
    x = np.asarray(superframe, dtype=np.uint8).reshape(-1)
    byte2 = int(x[2])
    n_aus, first = DABPLUS_FORMATS[((byte2 >> 6) & 1, (byte2 >> 5) & 1)]
    bits = np.unpackbits(x[:11])
    start = [first]
    for k in range(1, n_aus):
        t = 24 + 12 * (k - 1)
        start.append(int("".join(map(str, bits[t:t + 12])), 2))
    start.append(110 * int(s))
    consistent = all(start[k + 1] >= start[k] + 3 for k in range(n_aus))
    return bool(firecode_hit_numpy(x)), consistent, n_aus, start, byte2


def dabplus_au_table_numpy(superframes, s: int, rs_status=None):
    """the rule of vit_hip_dabplus_au_batch: superframes uint8 [...][>= 110 s], rs_status int [...][s] or None.  returns (info int64
    [...], au int64 [...][6][3] of (start, bytes, syndrome)); an entry without an access unit is (0, 0, 0xFFFFFFFF)"""
    x = np.asarray(superframes, dtype=np.uint8)
    s = int(s)
    if not 1 <= s <= 24 or x.shape[-1] < 110 * s:
        raise ValueError("outside the argument rule of vit_hip_dabplus_au_batch")
    lead = x.shape[:-1]
    flat = x.reshape(-1, x.shape[-1])
    status = None if rs_status is None else np.asarray(rs_status).reshape(-1, s)
    info = np.zeros(flat.shape[0], dtype=np.int64)
    au = np.zeros((flat.shape[0], 6, 3), dtype=np.int64)
    au[:, :, 2] = 0xFFFFFFFF
    for i, sf in enumerate(flat):
        fire_ok, consistent, n_aus, start, byte2 = dabplus_header_numpy(sf, s)
        valid = fire_ok and consistent
        failed = status is not None and bool((status[i] < 0).any())
        info[i] = int(fire_ok) | int(consistent) << 1 | int(failed) << 2 | (n_aus if valid else 0) << 4 | byte2 << 8
        if valid:
            for k in range(n_aus):
                n = start[k + 1] - start[k] - 2
                body = sf[start[k]:start[k] + n]
                field = int(sf[start[k] + n]) << 8 | int(sf[start[k] + n + 1])
                au[i, k] = (start[k], n, int(crc_numpy(DAB_CRC16, body, 8 * n)) ^ field)
    return info.reshape(lead), au.reshape(lead + (6, 3))


def dabplus_superframe_numpy(aus, dac_rate: int, sbr_flag: int, s: int, byte2_low: int = 0) -> np.ndarray:
    """the transmit side: the access units `aus` (a list of uint8 arrays: 2, 3, 4 or 6 of them by the format, at least one byte each,
    filling the 110 s data bytes exactly with their CRCs) -> the superframe as 5 logical frames, uint8 [5][24 s]: header (byte2_low
    fills bits 4 .. 0 of byte 2), access units with their CRC-16, Fire code, and the parity of the s RS(120,110) codewords"""
    s, dac_rate, sbr_flag = int(s), int(dac_rate) & 1, int(sbr_flag) & 1
    n_aus, first = DABPLUS_FORMATS[(dac_rate, sbr_flag)]
    aus = [np.asarray(a, dtype=np.uint8).reshape(-1) for a in aus]
    if not 1 <= s <= 24 or len(aus) != n_aus or any(a.size < 1 for a in aus):
        raise ValueError(f"this format has {n_aus} access units of at least one byte, s is 1 .. 24")
    if first + sum(a.size + 2 for a in aus) != 110 * s:
        raise ValueError(f"header, access units and their CRCs must fill {110 * s} bytes")
    data = np.zeros(110 * s, dtype=np.uint8)
    data[2] = dac_rate << 6 | sbr_flag << 5 | (int(byte2_low) & 0x1F)
    starts = first + np.concatenate([[0], np.cumsum([a.size + 2 for a in aus])])
    bits = np.unpackbits(data[:11])                                # the au_start fields end where access unit 0 begins
    for k in range(1, n_aus):
        bits[24 + 12 * (k - 1):24 + 12 * k] = [(int(starts[k]) >> (11 - j)) & 1 for j in range(12)]
    data[:11] = np.packbits(bits)
    for at, a in zip(starts, aus):
        crc = int(crc_numpy(DAB_CRC16, a, 8 * a.size))
        data[at:at + a.size] = a
        data[at + a.size], data[at + a.size + 1] = crc >> 8, crc & 0xFF
    fire = int(crc_numpy(FIRECODE, data[2:11], 72))
    data[0], data[1] = fire >> 8, fire & 0xFF
    return rs_encode_numpy(DABPLUS_RS_120_110, data, s).reshape(5, 24 * s)


class DabPlusDecoder:
    """the receiver of `rows` DAB+ sub-channels of one protection profile that move in lockstep: push(frames) takes the received soft bits
    [rows][F][n_received] on the device and returns (superframes, n_frames, info, au, rs_status) -- uint8 [rows][k][120 s] of which the
    first n_frames[r] (int32 [rows]) of row r are written, corrected in place; int32 [rows][k] and [rows][k][6][3] as
    BatchDecoder.dabplus_au_table returns them; int32 [rows][k][s] as rs_decode does -- all on the device, without a host
    synchronisation.  k is the capacity of the push, not a count.  The route: DabSubchannelDecoder.push -> dabplus_sync (running totals;
    frame0 = logical frames emitted so far mod 5) -> frames_extract (period 960 s, phase0 = frame0 * 192 s, the lock of the totals, the
    carry ping-ponged) -> rs_decode in place at interleave s -> dabplus_au_table.  Until a frame has hit, the lock names phase 0 with
    errors == compared and whatever is cut there shows fire_ok = 0.  `dec` is a BatchDecoder of the K = 7, R = 1/4 DAB code."""

    def __init__(self, dec, profile, rows: int = 1):
        s, rem = divmod(int(profile.info_bits), 192)
        if rem or not 1 <= s <= 24:
            raise ValueError("a DAB+ sub-channel carries 192 s bits a frame, s = 1 .. 24")
        self.dec, self.profile, self.rows, self.s = dec, profile, int(rows), s
        self.sub = DabSubchannelDecoder(dec, profile, rows)
        t, cb = dec.torch, (960 * s - 1 + 7) // 8
        self._totals = tuple(t.zeros(shape, dtype=t.int32, device=dec.device) for shape in ((self.rows, 5), (self.rows, 5), (self.rows, 4)))
        self._carry = [t.zeros((self.rows, cb), dtype=t.uint8, device=dec.device) for _ in range(2)]
        self._carry_bits = [t.zeros(self.rows, dtype=t.int32, device=dec.device) for _ in range(2)]
        self._cur = 0                                              # which of the two carries the next push reads
        self.emitted = 0                                           # logical frames seen so far: every row has the same

    @property
    def lock(self):
        """int32 CUDA [rows][4]: (phase in bits, 0, errors, compared) of the running totals"""
        return self._totals[2]

    def reset(self):
        """forget the totals, the carry and the de-interleaver's history"""
        self.sub.reset()
        for x in self._totals:
            x.zero_()
        self._carry_bits[self._cur].zero_()
        self.emitted = 0

    def push(self, frames):
        dec, t, s = self.dec, self.dec.torch, self.s
        logical = self.sub.push(frames)                            # [rows][nout][24 s]
        nout, B = int(logical.shape[1]), 24 * s
        if nout == 0:
            e = lambda *shape: t.empty((self.rows, 0) + shape, dtype=t.int32, device=dec.device)
            return t.empty((self.rows, 0, 5 * B), dtype=t.uint8, device=dec.device), t.zeros(self.rows, dtype=t.int32, device=dec.device), e(), e(6, 3), e(s)
        frame0 = self.emitted % 5
        dec.dabplus_sync(logical, frame_bytes=B, frame0=frame0, out=self._totals, accumulate=True)
        cur, nxt = self._cur, 1 - self._cur
        k = dec.frames_capacity(8 * B * nout, 40 * B)
        out = (t.empty((self.rows, k, 5 * B), dtype=t.uint8, device=dec.device), t.empty(self.rows, dtype=t.int32, device=dec.device), None,
               self._carry[nxt], self._carry_bits[nxt])
        sf, n_frames, _, _, _ = dec.frames_extract(logical.reshape(self.rows, nout * B), 8 * B * nout, 40 * B, frame0 * 8 * B, self._totals[2],
                                                   carry=self._carry[cur], carry_bits=self._carry_bits[cur], max_frames=k, out=out)
        self._cur = nxt
        self.emitted += nout
        sf, status = dec.rs_decode(DABPLUS_RS_120_110, sf, n_frames, interleave=s)
        info, au = dec.dabplus_au_table(sf, s, n_frames, status)
        return sf, n_frames, info, au, status
