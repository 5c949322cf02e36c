"""An independent statement of the Reed-Solomon rule of include/vit_hip.h, for the tests of BatchDecoder.rs_decode and of
viterbidecodercpp_amd.reed_solomon.  Nothing here is shared with the package: the field is a 256 x 256 product table made by
shift-and-add (no logarithms), the decoder is Peterson-Gorenstein-Zierler -- the largest e <= t whose e x e syndrome matrix is
regular gives the locator by Gaussian elimination, the error values come from a second linear system -- and its answer is accepted
only if it holds BY DEFINITION: every syndrome of the corrected word is zero and at most t bytes changed.  With e0 <= t errors the
matrices above e0 are singular and that of e0 is regular, so a codeword within t is always found; anything else fails the check."""
from functools import lru_cache

import numpy as np


@lru_cache(maxsize=None)
def mul_table(gfpoly):
    a = np.arange(256, dtype=np.int64)[:, None].repeat(256, axis=1)
    b = np.arange(256, dtype=np.int64)[None, :].repeat(256, axis=0)
    out = np.zeros((256, 256), dtype=np.int64)
    for _ in range(8):
        out ^= np.where(b & 1, a, 0)
        b >>= 1
        a <<= 1
        a ^= np.where(a & 0x100, gfpoly, 0)
    return out


def power(M, x, e):
    out = 1
    for _ in range(e):
        out = int(M[out, x])
    return out


def inverse(M, x):
    return int(np.flatnonzero(M[x] == 1)[0])


@lru_cache(maxsize=None)
def roots(gfpoly, fcr, prim, nroots):
    M = mul_table(gfpoly)
    return [power(M, 2, prim * (fcr + j) % 255) for j in range(nroots)]


@lru_cache(maxsize=None)
def dual_tables(gfpoly):
    """(to_dual, to_conv): bit 7-i of the stored byte is Tr(x beta^i), beta = alpha^117"""
    M = mul_table(gfpoly)
    beta = power(M, 2, 117)
    to_dual = np.zeros(256, dtype=np.uint8)
    for x in range(256):
        stored, y = 0, x
        for i in range(8):
            tr, p = 0, y
            for _ in range(8):
                tr ^= p
                p = int(M[p, p])
            assert tr in (0, 1)
            stored |= tr << (7 - i)
            y = int(M[y, beta])
        to_dual[x] = stored
    to_conv = np.zeros(256, dtype=np.uint8)
    to_conv[to_dual] = np.arange(256)
    return to_dual, to_conv


def syndromes(M, rts, word):
    s = np.zeros(len(rts), dtype=np.int64)
    r = np.asarray(rts)
    for byte in word:
        s = M[s, r] ^ int(byte)
    return s


def solve(M, A, b):
    """x with A x = b over the field, or None when A is singular"""
    e = len(b)
    A = np.concatenate([np.asarray(A, dtype=np.int64), np.asarray(b, dtype=np.int64)[:, None]], axis=1)
    for col in range(e):
        piv = next((r for r in range(col, e) if A[r, col]), None)
        if piv is None:
            return None
        A[[col, piv]] = A[[piv, col]]
        A[col] = M[A[col], inverse(M, int(A[col, col]))]
        for r in range(e):
            if r != col and A[r, col]:
                A[r] ^= M[A[col], A[r, col]]
    return A[:, e]


def decode_word(gfpoly, fcr, prim, nroots, word):
    """word: conventional symbols [n] -> (word, status)"""
    M = mul_table(gfpoly)
    rts = roots(gfpoly, fcr, prim, nroots)
    n, t = len(word), nroots // 2
    word = np.asarray(word, dtype=np.int64)
    S = syndromes(M, rts, word)
    if not S.any():
        return word, 0
    gamma = power(M, 2, prim)
    X = [power(M, gamma, n - 1 - i) for i in range(n)]            # the locator of byte i, the power x^(n-1-i)
    for e in range(t, 0, -1):
        lam = solve(M, [[S[i + j] for j in range(e)] for i in range(e)], [S[e + i] for i in range(e)])   # lam[j] = Lambda_(e-j)
        if lam is None:
            continue
        where = []
        for i in range(n):                                        # Lambda(1 / X_i) = 0  <=>  X_i^e + Lambda_1 X_i^(e-1) + ... + Lambda_e = 0
            acc = 1
            for j in range(e - 1, -1, -1):
                acc = int(M[acc, X[i]]) ^ int(lam[j])
            if acc == 0:
                where.append(i)
        if len(where) != e:
            break
        first = [power(M, X[i], fcr) for i in where]
        rows, col = [], list(first)
        for j in range(e):                                        # sum_k Y_k X_k^(fcr + j) = S_j
            rows.append(list(col))
            col = [int(M[c, X[i]]) for c, i in zip(col, where)]
        Y = solve(M, rows, S[:e])
        if Y is None:
            break
        fixed = word.copy()
        fixed[where] ^= Y
        changed = int((fixed != word).sum())
        if changed <= t and not syndromes(M, rts, fixed).any():
            return fixed, changed
        break
    return word, -1


def decode(code, frames, interleave=1):
    """code: anything with gfpoly, fcr, prim, nroots, pad, dual_basis.  frames uint8 [..., n I] -> (frames, status int32 [..., I])"""
    frames = np.asarray(frames, dtype=np.uint8)
    n, I = 255 - code.pad, int(interleave)
    lead = frames.shape[:-1]
    flat = frames.reshape(-1, n * I)
    out = flat.copy()
    status = np.zeros((flat.shape[0], I), dtype=np.int32)
    to_dual, to_conv = dual_tables(code.gfpoly) if code.dual_basis else (np.arange(256, dtype=np.uint8),) * 2
    for m in range(flat.shape[0]):
        for c in range(I):
            word, status[m, c] = decode_word(code.gfpoly, code.fcr, code.prim, code.nroots, to_conv[flat[m, c::I]])
            out[m, c::I] = to_dual[word.astype(np.uint8)]
    return out.reshape(frames.shape), status.reshape(lead + (I,))


def corrupt(rng, frame, interleave, c, count, where="any", n=None, nroots=None):
    """`count` distinct byte errors in codeword c of `frame` (in place): where = any | first (position 0 on) | last (n-1 back) |
    parity | data"""
    I = int(interleave)
    n = frame.size // I if n is None else n
    if where == "first":
        pos = np.arange(count)
    elif where == "last":
        pos = n - 1 - np.arange(count)
    elif where == "parity":
        pos = n - nroots + rng.choice(nroots, size=count, replace=False)
    elif where == "data":
        pos = rng.choice(n - nroots, size=count, replace=False)
    else:
        pos = rng.choice(n, size=count, replace=False)
    frame[pos * I + c] ^= rng.integers(1, 256, size=count).astype(np.uint8)
    return pos
