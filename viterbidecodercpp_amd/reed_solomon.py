"""Reed-Solomon codes over GF(256) (BatchDecoder.rs_decode / vit_hip_rs_decode_batch): the parameters, the stock codes of the links this
project names, and the rule in numpy.

A code is described as libfec describes one: the field polynomial `gfpoly` (alpha = 0x02), the generator's roots alpha^(prim (fcr + j)),
0 <= j < nroots, `pad` symbols of virtual fill (n = 255 - pad are transmitted) and the CCSDS dual basis on or off.  A codeword is the
bytes c_0 .. c_(n-1) with c_0 the coefficient of x^(n-1): data first, parity last.  With interleave depth I a frame is n * I bytes and
symbol i of codeword c is frame byte i * I + c.  `rs_encode_numpy` and `rs_decode_numpy` restate the rule of include/vit_hip.h on the
host, as frame_sync.frames_extract_numpy restates the extraction: the decoder gives the one valid codeword within t = nroots // 2 byte
errors of what it received with the number of errors as status, or the received word unchanged and status -1.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np


@dataclass(frozen=True)
class RSCode:
    """the parameters of vit_hip_rs_params"""
    gfpoly: int
    fcr: int
    prim: int
    nroots: int
    pad: int = 0
    dual_basis: bool = False

    def __post_init__(self):
        if not 0x100 <= self.gfpoly <= 0x1FF or not 2 <= self.nroots <= 64 or not 0 <= self.pad < 255 or 255 - self.pad <= self.nroots:
            raise ValueError("gfpoly needs its x^8 term, nroots is 2 .. 64, n = 255 - pad exceeds nroots")
        if not 1 <= self.prim <= 254 or np.gcd(self.prim, 255) != 1 or not 0 <= self.fcr <= 254:
            raise ValueError("prim is 1 .. 254 and coprime to 255, fcr is 0 .. 254")
        if self.dual_basis and self.gfpoly != 0x187:
            raise ValueError("the dual basis is defined for gfpoly 0x187 only")
        _field(self.gfpoly)

    @property
    def n(self) -> int:
        return 255 - self.pad

    @property
    def k(self) -> int:
        return self.n - self.nroots

    @property
    def t(self) -> int:
        return self.nroots // 2


@lru_cache(maxsize=None)
def _field(gfpoly: int):
    """(exp [510], log [256]) of GF(2)[x] / gfpoly with alpha = x; raises unless x is primitive"""
    exp, log = np.zeros(510, dtype=np.int64), np.zeros(256, dtype=np.int64)
    v = 1
    for i in range(255):
        if i and v == 1:
            raise ValueError(f"gfpoly {gfpoly:#x} is not primitive")
        exp[i], log[v] = v, i
        v <<= 1
        if v & 0x100:
            v ^= gfpoly
    if v != 1:
        raise ValueError(f"gfpoly {gfpoly:#x} is not primitive")
    exp[255:] = exp[:255]
    return exp, log


CCSDS_RS_255_223 = RSCode(0x187, 112, 11, 32)
CCSDS_RS_255_239 = RSCode(0x187, 120, 11, 16)
CCSDS_RS_255_223_DUAL = RSCode(0x187, 112, 11, 32, dual_basis=True)
CCSDS_RS_255_239_DUAL = RSCode(0x187, 120, 11, 16, dual_basis=True)
DVB_RS_204_188 = RSCode(0x11D, 0, 1, 16, pad=51)


def _mul(field, a, b):
    exp, log = field
    return int(exp[log[a] + log[b]]) if a and b else 0


@lru_cache(maxsize=None)
def dual_basis_tables(gfpoly: int = 0x187):
    """(to_dual, to_conv) uint8 [256]: conventional x is stored as the byte whose bit 7-i is Tr(x beta^i), beta = alpha^117"""
    exp, log = _field(gfpoly)
    to_dual, to_conv = np.zeros(256, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    for x in range(1, 256):
        stored = 0
        for i in range(8):
            y = int(exp[(log[x] + 117 * i) % 255])
            tr, p = 0, y
            for _ in range(8):
                tr ^= p
                p = _mul((exp, log), p, p)
            stored |= (tr & 1) << (7 - i)
        to_dual[x] = stored
    to_conv[to_dual] = np.arange(256, dtype=np.uint8)
    return to_dual, to_conv


@lru_cache(maxsize=None)
def generator(code: RSCode) -> tuple:
    """the generator polynomial's coefficients, low to high (nroots + 1 of them; the highest is 1)"""
    f = _field(code.gfpoly)
    g = [1]
    for j in range(code.nroots):
        root = int(f[0][code.prim * (code.fcr + j) % 255])
        g = [(g[i - 1] if i else 0) ^ _mul(f, g[i] if i < len(g) else 0, root) for i in range(len(g) + 1)]
    return tuple(g)


def _codewords(code: RSCode, frames, interleave: int, width: int):
    """frames [..., width * I] -> [m][I][width] (a copy), and the leading shape"""
    frames = np.asarray(frames, dtype=np.uint8)
    I = int(interleave)
    if I < 1 or frames.shape[-1] != width * I:
        raise ValueError(f"the last dimension must be {width} * interleave")
    lead = frames.shape[:-1]
    return frames.reshape(-1, width, I).transpose(0, 2, 1).copy(), lead


def rs_encode_numpy(code: RSCode, data, interleave: int = 1) -> np.ndarray:
    """data uint8 [..., k * I], interleaved like a frame -> frames uint8 [..., n * I]: systematic, the parity of every codeword behind
    its data.  With dual_basis, data and frames are stored (Berlekamp) symbols."""
    f = _field(code.gfpoly)
    g = generator(code)
    words, lead = _codewords(code, data, interleave, code.k)
    if code.dual_basis:
        to_dual, to_conv = dual_basis_tables(code.gfpoly)
        words = to_conv[words]
    out = np.zeros(words.shape[:2] + (code.n,), dtype=np.uint8)
    out[..., :code.k] = words
    for w in out.reshape(-1, code.n):
        reg = [0] * code.nroots                                   # the remainder of data(x) x^nroots by g, highest coefficient first
        for byte in w[:code.k]:
            fb = int(byte) ^ reg[0]
            reg = [reg[i + 1] ^ _mul(f, fb, g[code.nroots - 1 - i]) for i in range(code.nroots - 1)] + [_mul(f, fb, g[0])]
        w[code.k:] = reg
    if code.dual_basis:
        out = to_dual[out]
    return out.transpose(0, 2, 1).reshape(lead + (code.n * int(interleave),))


def syndromes(code: RSCode, word) -> list:
    """S_j = word(alpha^(prim (fcr + j))) of ONE codeword in conventional symbols"""
    exp, log = _field(code.gfpoly)
    rootlog = code.prim * (code.fcr + np.arange(code.nroots)) % 255
    s = np.zeros(code.nroots, dtype=np.int64)
    for byte in word:                                             # Horner's rule at all roots at once
        s = np.where(s != 0, exp[log[s] + rootlog], 0) ^ int(byte)
    return [int(x) for x in s]


def _decode_word(code: RSCode, f, word):
    """word: conventional symbols, corrected in place; returns the status"""
    exp, log = f
    n, nroots, prim, fcr = code.n, code.nroots, code.prim, code.fcr
    S = syndromes(code, word)
    if not any(S):
        return 0
    # Berlekamp-Massey
    lam, B, L = [1] + [0] * nroots, [1] + [0] * nroots, 0
    for r in range(nroots):
        B = [0] + B[:-1]
        d = 0
        for i in range(min(r, L) + 1):
            d ^= _mul(f, lam[i], S[r - i])
        if d:
            nxt = [lam[i] ^ _mul(f, d, B[i]) for i in range(nroots + 1)]
            if 2 * L <= r:
                inv = int(exp[255 - log[d]])
                B = [_mul(f, x, inv) for x in lam]
                L = r + 1 - L
            lam = nxt
    deg = max(i for i, x in enumerate(lam) if x)
    if deg != L or L > code.t:
        return -1
    omega = [0] * L
    for i in range(L):
        for m in range(i + 1):
            omega[i] ^= _mul(f, lam[m], S[i - m])
    # position p is the power of x: X = alpha^(prim p), z = 1 / X; all 255 values of z at once
    zl = prim * ((255 - np.arange(255)) % 255) % 255
    total, odd, om = (np.zeros(255, dtype=np.int64) for _ in range(3))
    for i in range(L + 1):
        if lam[i]:
            term = exp[(log[lam[i]] + i * zl) % 255]
            total ^= term
            if i & 1:
                odd ^= term
        if i < L and omega[i]:
            om ^= exp[(log[omega[i]] + i * zl) % 255]
    fixes = []
    for p in np.flatnonzero(total == 0):
        if p >= n or om[p] == 0 or odd[p] == 0:
            return -1
        # Forney: Y = X^(-fcr) Omega(z) / (z Lambda'(z)), and z Lambda'(z) is the odd part of Lambda(z)
        fixes.append((n - 1 - int(p), int(exp[(log[om[p]] + 255 - log[odd[p]] + int(zl[p]) * fcr) % 255])))
    if len(fixes) != L:
        return -1
    for i, y in fixes:
        word[i] ^= y
    return L


def rs_decode_numpy(code: RSCode, frames, interleave: int = 1):
    """the rule of vit_hip_rs_decode_batch: frames uint8 [..., n * I] -> (frames of the same shape, status int32 [..., I])"""
    f = _field(code.gfpoly)
    words, lead = _codewords(code, frames, interleave, code.n)
    if code.dual_basis:
        to_dual, to_conv = dual_basis_tables(code.gfpoly)
        words = to_conv[words]
    status = np.zeros(words.shape[:2], dtype=np.int32)
    for m in range(words.shape[0]):
        for c in range(words.shape[1]):
            w = words[m, c].astype(np.int64)
            status[m, c] = _decode_word(code, f, w)
            words[m, c] = w
    if code.dual_basis:
        words = to_dual[words]
    return words.transpose(0, 2, 1).reshape(lead + (code.n * int(interleave),)), status.reshape(lead + (int(interleave),))
