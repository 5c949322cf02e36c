"""The DAB receive chain around the K = 7, R = 1/4 decoder (ETSI EN 300 401): the puncturing vectors and profiles of clause 11, the time
interleaver of clause 12 and the energy dispersal of clause 10 -- the maps vit_hip_dab_deinterleave_batch takes, the rules of the receive
side on the host (dab_time_deinterleave_numpy, dab_depuncture_numpy, dab_energy_dispersal_numpy), the transmit side
(dab_time_interleave_numpy, dab_puncture_numpy) and the sub-channel receiver DabSubchannelDecoder.  The GPU side is
BatchDecoder.dab_deinterleave (decoder.py) and BatchDecoder.dab_descramble (outer.py).  The unequal-error-protection table is not here: a
UEP row is any list of segments."""
from __future__ import annotations

import numpy as np

DAB_HISTORY_FRAMES = 15
DAB_PRBS_PERIOD = 511
# the delay of soft bit i in frames is DAB_DELAYS[i mod 16]: the 4-bit reversal
DAB_DELAYS = (0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15)
# the order in which the positions of a 32-entry vector are added to the always-kept 0, 4, ..., 28
_ADD_ORDER = tuple(c + 4 * g for c in (1, 2, 3) for g in (0, 4, 2, 6, 1, 5, 3, 7))


def puncture_vector(i: int) -> np.ndarray:
    """PI_i, i = 1 .. 24: bool [32] with 8 + i ones; the vectors are nested (PI_8 = 1100 eight times, PI_16 = 1110 eight times)"""
    i = int(i)
    if not 1 <= i <= 24:
        raise ValueError("the puncturing index must be 1 .. 24")
    v = np.zeros(32, dtype=bool)
    v[0::4] = True
    v[list(_ADD_ORDER[:i])] = True
    return v


PI_X = np.tile(np.array([1, 1, 0, 0], dtype=bool), 6)             # the 24 tail symbols: 12 kept


class DabProfile:
    """a protection profile: segments = [(blocks, pi), ...], `blocks` blocks of 128 mother-code symbols (32 information bits) punctured
    with PI_pi, the 32-entry vector four times a block, then the 24-symbol tail with PI_X.  info_bits = I = 32 sum(blocks), steps = S = I
    + 6, symbols_per_frame = 4 S, n_received = the symbols kept = sum(blocks 4 (8 + pi)) + 12"""

    def __init__(self, segments):
        self.segments = tuple((int(b), int(p)) for b, p in segments)
        if not self.segments or any(b < 1 or not 1 <= p <= 24 for b, p in self.segments):
            raise ValueError("segments must be (blocks >= 1, puncturing index 1 .. 24) pairs")
        self.info_bits = 32 * sum(b for b, _ in self.segments)
        self.steps = self.info_bits + 6
        self.symbols_per_frame = 4 * self.steps
        self.n_received = sum(b * 4 * (8 + p) for b, p in self.segments) + 12

    def mask(self) -> np.ndarray:
        """bool [symbols_per_frame]: the mother-code symbols that are sent"""
        return np.concatenate([np.tile(puncture_vector(p), 4 * b) for b, p in self.segments] + [PI_X])

    def source_index(self) -> np.ndarray:
        """int32 [symbols_per_frame]: the received soft bit every mother-code symbol is, -1 where it was punctured -- d_source_index"""
        m = self.mask()
        return np.where(m, np.cumsum(m) - 1, -1).astype(np.int32)

    def __repr__(self):
        return f"DabProfile({list(self.segments)})"


FIC_PROFILE = DabProfile([(21, 16), (3, 15)])                      # 768 bits from 2304 symbols: the Fast Information Channel, mode I


def eep_profile(level: str, n: int) -> DabProfile:
    """the equal-error-protection profile `level` ("1-A" .. "4-A" at 8 n kbit/s, I = 192 n; "1-B" .. "4-B" at 32 n kbit/s, I = 768 n)"""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    a = {"1-A": [(6 * n - 3, 24), (3, 23)],
         "2-A": [(5, 13), (1, 12)] if n == 1 else [(2 * n - 3, 14), (4 * n + 3, 13)],
         "3-A": [(6 * n - 3, 8), (3, 7)],
         "4-A": [(4 * n - 3, 3), (2 * n + 3, 2)]}
    b = {"1-B": 10, "2-B": 6, "3-B": 4, "4-B": 2}
    if level in a:
        return DabProfile(a[level])
    if level in b:
        return DabProfile([(24 * n - 3, b[level]), (3, b[level] - 1)])
    raise ValueError("level must be 1-A .. 4-A or 1-B .. 4-B")


def dab_prbs(n_bits: int) -> np.ndarray:
    """the first n_bits bits of the energy-dispersal sequence, uint8 [n_bits]: p[n] = p[n-5] ^ p[n-9], p[-9 .. -1] = 1 (period 511;
    as bytes 07 BE 2E 64 12 9D A3 CF ...)"""
    p = np.ones(DAB_PRBS_PERIOD + 9, dtype=np.uint8)
    for k in range(9, DAB_PRBS_PERIOD + 9):
        p[k] = p[k - 5] ^ p[k - 9]
    return p[9:][np.arange(int(n_bits)) % DAB_PRBS_PERIOD]


def dab_energy_dispersal_numpy(frames, n_bits: int = None) -> np.ndarray:
    """the rule of vit_hip_dab_descramble_batch on the host (and the transmit side: dispersal is its own inverse): frames uint8 [...][>=
    ceil(n_bits/8)] -> [...][ceil(n_bits/8)], bit t < n_bits of every frame XORed with the sequence; n_bits defaults to all bits"""
    x = np.asarray(frames, dtype=np.uint8)
    n_bits = 8 * x.shape[-1] if n_bits is None else int(n_bits)
    nb = (n_bits + 7) // 8
    if x.shape[-1] < nb:
        raise ValueError(f"{n_bits} bits need {nb} bytes per frame")
    bits = np.zeros(8 * nb, dtype=np.uint8)
    bits[:n_bits] = dab_prbs(n_bits)
    return x[..., :nb] ^ np.packbits(bits)


def dab_puncture_numpy(coded, profile: DabProfile) -> np.ndarray:
    """the transmit side: coded [F][S][4] (or [F][4 S]) -> [F][n_received], the symbols the profile keeps"""
    x = np.asarray(coded)
    x = x.reshape(x.shape[0], -1)
    if x.shape[1] != profile.symbols_per_frame:
        raise ValueError(f"a codeword of this profile has {profile.symbols_per_frame} symbols")
    return np.ascontiguousarray(x[:, profile.mask()])


def dab_depuncture_numpy(received, profile: DabProfile) -> np.ndarray:
    """the rule of the map on the host: received [F][n_received] -> [F][S][4], 0 (the erasure) where nothing was sent"""
    x = np.asarray(received)
    if x.ndim != 2 or x.shape[1] != profile.n_received:
        raise ValueError(f"a frame of this profile has {profile.n_received} received symbols")
    idx = profile.source_index()
    out = np.where(idx >= 0, x[:, np.maximum(idx, 0)], 0).astype(x.dtype)
    return out.reshape(x.shape[0], profile.steps, 4)


def dab_time_interleave_numpy(frames) -> np.ndarray:
    """the transmit side: logical frames a [N][n] -> sent frames b [N][n], b[r][i] = a[r - d(i mod 16)][i]; 0 where r - d < 0"""
    a = np.asarray(frames)
    N, n = a.shape
    src = np.arange(N)[:, None] - np.asarray(DAB_DELAYS)[np.arange(n) % 16][None, :]
    return np.where(src >= 0, a[np.maximum(src, 0), np.arange(n)[None, :]], 0).astype(a.dtype)


def dab_time_deinterleave_numpy(frames, hist=None, fill: int = 0, n_frames: int = None):
    """the rule of vit_hip_dab_deinterleave_batch (identity map) for ONE row: frames [>= nf][n], hist [15][n] or None, of which the last
    min(fill, 15) frames are real.  returns (out [nout][n], nout, hist [15][n] -- the frames in front of the real ones zero --, fill)"""
    x = np.asarray(frames)
    H, n = DAB_HISTORY_FRAMES, int(x.shape[1])
    nf = x.shape[0] if n_frames is None else min(int(n_frames), x.shape[0])
    fill = min(int(fill), H) if hist is not None else 0
    old = np.asarray(hist, dtype=x.dtype).reshape(H, n)[H - fill:] if fill else np.zeros((0, n), dtype=x.dtype)
    S = np.concatenate([old, x[:nf]])
    T = S.shape[0]
    nout = max(0, T - H)
    i = np.arange(n)
    d = np.asarray(DAB_DELAYS)[i % 16]
    out = np.zeros((nout, n), dtype=x.dtype)
    for k in range(nout):
        out[k] = S[k + d, i]
    keep = min(H, T)
    new = np.zeros((H, n), dtype=x.dtype)
    if keep:
        new[H - keep:] = S[T - keep:]
    return out, nout, new, keep


class DabSubchannelDecoder:
    """the receiver of `rows` sub-channels of one protection profile that move in lockstep: push(frames) takes the received soft bits
    [rows][F][n_received] on the device (any F; a view into whole CIFs is fine) and returns the decoded, descrambled bytes
    [rows][nout][I/8] of the logical frames this push completed -- nothing until 15 frames are in.  It owns the ping-ponged history; the
    route is BatchDecoder.dab_deinterleave (with the profile's map) -> decode(L = I) -> dab_descramble, all on the current stream.
    `dec` is a BatchDecoder of the K = 7, R = 1/4 DAB code."""

    def __init__(self, dec, profile: DabProfile, rows: int = 1):
        if dec.R != 4:
            raise ValueError("the DAB mother code has rate 1/4")
        self.dec, self.profile, self.rows = dec, profile, int(rows)
        if self.rows < 1:
            raise ValueError("rows must be at least 1")
        t = dec.torch
        self._map = t.from_numpy(profile.source_index()).to(dec.device)
        n = profile.n_received
        self._hist = [t.zeros((self.rows, DAB_HISTORY_FRAMES * n), dtype=dec._soft_dtype, device=dec.device) for _ in range(2)]
        self._fill = [t.zeros(self.rows, dtype=t.int32, device=dec.device) for _ in range(2)]
        self._n_out = t.zeros(self.rows, dtype=t.int32, device=dec.device)
        self._cur = 0                                              # which of the two histories the next push reads
        self.fill = 0                                              # the host's copy of the fill: every row has the same

    def reset(self):
        """forget the history: the next 15 frames pushed complete nothing"""
        self._fill[self._cur].zero_()
        self.fill = 0

    def push(self, frames):
        dec, p, t = self.dec, self.profile, self.dec.torch
        if frames.dim() == 2:
            frames = frames.unsqueeze(0)
        if frames.dim() != 3 or frames.shape[0] != self.rows or frames.shape[2] < p.n_received:
            raise ValueError(f"frames must be [{self.rows}][F][>= {p.n_received}]")
        F = int(frames.shape[1])
        nb = p.info_bits // 8
        if F == 0:
            return t.empty((self.rows, 0, nb), dtype=t.uint8, device=dec.device)
        cur, nxt = self._cur, 1 - self._cur
        sym = t.empty((self.rows, F, p.symbols_per_frame), dtype=dec._soft_dtype, device=dec.device)
        dec.dab_deinterleave(frames, source_index=self._map, hist=self._hist[cur], fill=self._fill[cur], n_received=p.n_received,
                             out=(sym, self._n_out, self._hist[nxt], self._fill[nxt]))
        self._cur = nxt
        T = self.fill + F
        nout = max(0, T - DAB_HISTORY_FRAMES)
        self.fill = min(T, DAB_HISTORY_FRAMES)
        if nout == 0:
            return t.empty((self.rows, 0, nb), dtype=t.uint8, device=dec.device)
        done = sym[:, :nout].reshape(self.rows * nout, p.steps, 4)  # a view once the history is full (nout == F), else a copy
        out = dec.decode(done.contiguous(), p.info_bits)
        return dec.dab_descramble(out, p.info_bits, in_place=True).reshape(self.rows, nout, nb)
