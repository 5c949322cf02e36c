"""The rule of vit_hip_frames_extract (include/vit_hip.h) written a second time, independently of
viterbidecodercpp_amd.frame_sync.frames_extract_numpy: by plain loops over bit positions (`extract_loop`), and through Python's long
integers for the larger cases (`extract_ints`: a row is one integer, a frame a shift and a mask); the makers of the cases the CPU and
GPU tests share; and the images the output buffers of a call must equal byte for byte, written and unwritten bytes alike."""
import numpy as np


def bit(buf, t):
    return (int(buf[t >> 3]) >> (7 - (t & 7))) & 1


def cut(P, phase0, phase, c, n_bits):
    """(skip, nf, rem) of one row"""
    skip = (phase % P + c - phase0) % P
    total = c + n_bits
    if skip >= total:
        return skip, 0, 0
    return skip, (total - skip) // P, (total - skip) % P


def pack(bits):
    out = bytearray((len(bits) + 7) // 8)
    for k, b in enumerate(bits):
        if b:
            out[k >> 3] |= 0x80 >> (k & 7)
    return np.frombuffer(bytes(out), dtype=np.uint8)


def extract_loop(row, n_bits, P, phase0, phase, inverted, carry=None, c=0, marker=0, m=0, d=0, pad=None):
    """one row, bit by bit: (frames [nf][ceil(Q/8)] uint8, errors [nf] list (m > 0) or None, carry_out uint8 [ceil(rem/8)], rem)"""
    c = 0 if carry is None or c > P - 1 else c
    S = [bit(carry, t) for t in range(c)] + [bit(row, t) for t in range(n_bits)]
    skip, nf, rem = cut(P, phase0, phase, c, n_bits)
    inv = 1 if inverted else 0
    Q = P - d
    frames, errors = np.zeros((nf, (Q + 7) // 8), dtype=np.uint8), []
    for f in range(nf):
        F = [S[skip + f * P + j] ^ inv for j in range(P)]
        errors.append(sum(F[j] != ((marker >> (m - 1 - j)) & 1) for j in range(m)))
        frames[f] = pack([F[d + k] ^ (bit(pad, k) if pad is not None else 0) for k in range(Q)])
    return frames, (errors if m else None), pack(S[skip + nf * P:skip + nf * P + rem]), rem


def extract_ints(row, n_bits, P, phase0, phase, inverted, carry=None, c=0, marker=0, m=0, d=0, pad=None):
    """the same through long integers: the logical stream is ONE integer whose highest bit is stream bit 0"""
    c = 0 if carry is None or c > P - 1 else c
    nb, cb = (n_bits + 7) // 8, (c + 7) // 8
    S = int.from_bytes(bytes(row[:nb]), "big") >> (8 * nb - n_bits)
    if c:
        S |= (int.from_bytes(bytes(carry[:cb]), "big") >> (8 * cb - c)) << n_bits
    total = c + n_bits
    take = lambda at, n: (S >> (total - at - n)) & ((1 << n) - 1)        # stream bits [at, at + n) as an n-bit integer
    skip, nf, rem = cut(P, phase0, phase, c, n_bits)
    Q = P - d
    qb = (Q + 7) // 8
    padv = int.from_bytes(bytes(pad[:qb]), "big") >> (8 * qb - Q) if pad is not None else 0
    frames, errors = np.zeros((nf, qb), dtype=np.uint8), []
    for f in range(nf):
        F = take(skip + f * P, P) ^ (((1 << P) - 1) if inverted else 0)
        errors.append(bin((F >> (P - m)) ^ marker).count("1") if m else 0)
        out = ((F & ((1 << Q) - 1)) ^ padv) << (8 * qb - Q)
        frames[f] = np.frombuffer(out.to_bytes(qb, "big"), dtype=np.uint8)
    rb = (rem + 7) // 8
    carry_out = np.frombuffer((take(skip + nf * P, rem) << (8 * rb - rem)).to_bytes(rb, "big"), dtype=np.uint8) if rem else np.zeros(0, np.uint8)
    return frames, (errors if m else None), carry_out, rem


def capacity(n_bits, P):
    return (n_bits + P - 1) // P


def make_case(seed, rows, n_bits, P, phase0=0, c=0, skip=None, phase=None, inverted=0, d=0, m=0, marker=None, pad=False, stride_extra=0,
              carry_extra=0, frame_extra=0, max_extra=0, carry=True, phase_plus=0):
    """a random case.  c: the carry length of every row, or one per row (values above P-1 are kept: the rule reads them as 0).  skip:
    aim the lock of every row at that skip (phase = skip + phase0 - c mod P), or give `phase`; phase_plus is added to it (a multiple of
    P changes nothing: the rule takes the phase mod P).  The pad bits of the last byte of rows and carries and the bytes behind them are random: the rule never reads them."""
    rng = np.random.default_rng(seed)
    nb, cb = (n_bits + 7) // 8, (P + 6) // 8
    cs = np.broadcast_to(np.asarray(c, dtype=np.int64), (rows,)).copy()
    lock = np.zeros((rows, 4), dtype=np.int64)
    for r in range(rows):
        ce = 0 if (not carry or cs[r] > P - 1) else int(cs[r])
        ph = int(rng.integers(0, P)) if skip is None and phase is None else (phase if phase is not None else (skip + phase0 - ce) % P)
        lock[r] = (ph + phase_plus, inverted if inverted in (0, 1) else int(rng.integers(0, 2)), int(rng.integers(0, 1000)), int(rng.integers(0, 1000)))
    Q = P - d
    if marker is None:
        marker = int.from_bytes(rng.bytes(8), "big") & ((1 << m) - 1) if m else 0
    return dict(rows=rows, n_bits=n_bits, P=P, phase0=phase0, d=d, m=m, marker=marker, Q=Q, qb=(Q + 7) // 8, nb=nb, cb=cb,
                stride=nb + stride_extra, cstride=cb + carry_extra, fstride=(Q + 7) // 8 + frame_extra,
                max_frames=capacity(n_bits, P) + max_extra,
                bytes=rng.integers(0, 256, size=(rows, nb + stride_extra), dtype=np.uint8),
                carry=rng.integers(0, 256, size=(rows, cb + carry_extra), dtype=np.uint8) if carry else None, carry_bits=cs, lock=lock,
                pad=rng.integers(0, 256, size=(Q + 7) // 8, dtype=np.uint8) if pad else None)


def case_reference(c, form=extract_ints):
    """per row (frames, errors, carry_out, rem) of a case of make_case"""
    return [form(c["bytes"][r], c["n_bits"], c["P"], c["phase0"], int(c["lock"][r, 0]), int(c["lock"][r, 1]),
                 None if c["carry"] is None else c["carry"][r], int(c["carry_bits"][r]), c["marker"], c["m"], c["d"], c["pad"])
            for r in range(c["rows"])]


def images(c, ref, poison=0xA5):
    """what the five outputs must hold after a call on buffers filled with `poison` bytes: (frames uint8 [rows * max_frames * fstride],
    n_frames uint32 [rows], marker_errors uint32 [rows * max_frames], carry_out uint8 [rows * cstride], carry_bits_out uint32 [rows]) --
    frames >= nf, the bytes behind a frame in its stride, the distances of unwritten frames and the bytes behind a carry keep the poison"""
    rows, mf, fs, cs, qb = c["rows"], c["max_frames"], c["fstride"], c["cstride"], c["qb"]
    word = poison * 0x01010101
    frames = np.full(rows * mf * fs, poison, dtype=np.uint8)
    errors = np.full(rows * mf, word, dtype=np.uint32)
    carry = np.full(rows * cs, poison, dtype=np.uint8)
    n, bits = np.zeros(rows, dtype=np.uint32), np.zeros(rows, dtype=np.uint32)
    for r, (fr, er, co, rem) in enumerate(ref):
        n[r], bits[r] = len(fr), rem
        for f in range(len(fr)):
            at = (r * mf + f) * fs
            frames[at:at + qb] = fr[f]
            if er is not None:
                errors[r * mf + f] = er[f]
        carry[r * cs:r * cs + len(co)] = co
    return frames, n, errors, carry, bits


# ---- the receiver: search, lock, extract per internal call --------------------------------------------------------------------

def framed_stream(seed, marker, m, P, n_frames, lead, pad=None, trail=0):
    """(bits 0/1 uint8, payloads uint8 [n_frames][(P - m) / 8]): `lead` random bits, then n_frames frames of the marker and a random
    payload XORed with `pad` (the transmitter randomises, the receiver's pad takes it off again), then `trail` random bits"""
    rng = np.random.default_rng(seed)
    payload = rng.integers(0, 256, size=(n_frames, (P - m) // 8), dtype=np.uint8)
    sent = payload if pad is None else payload ^ np.asarray(pad, dtype=np.uint8)[:payload.shape[1]]
    mk = np.array([(marker >> (m - 1 - j)) & 1 for j in range(m)], dtype=np.uint8)
    frames = np.concatenate([np.broadcast_to(mk, (n_frames, m)), np.unpackbits(sent, axis=1)], axis=1)
    lead_bits, trail_bits = rng.integers(0, 2, size=lead, dtype=np.uint8), rng.integers(0, 2, size=trail, dtype=np.uint8)
    return np.concatenate([lead_bits, frames.reshape(-1), trail_bits]), payload


def receiver_numpy(bits, chunks, marker, m, P, d=0, pad=None):
    """what a receiver with frames=True does, in numpy, over the calls that emit `chunks` bits each: accumulate the marker totals
    (history = the last m-1 emitted bits), take the lock of the totals, extract under it with the carry of the call before.  returns
    (frames uint8 [n][ceil((P-d)/8)], marker_errors int64 [n], locks [(phase, inverted)] of the call that completed each frame)"""
    from viterbidecodercpp_amd import frame_sync as fs
    distance, count = np.zeros((1, P), dtype=np.int64), np.zeros((1, P), dtype=np.int64)
    lock = np.zeros(4, dtype=np.int64)
    carry, cbits, at = None, 0, 0
    frames, errors, locks = [], [], []
    for n in chunks:
        seg = bits[at:at + n]
        hb = min(m - 1, at)
        if n + hb >= m:
            hist = int("".join(map(str, bits[at - hb:at])), 2) if hb else 0
            dd, cc = fs.marker_search_numpy(np.packbits(seg), n, marker, m, P, at % P, [hist], hb)
            distance, count = distance + dd, count + cc
            lock = fs.marker_lock_numpy(distance, count, m)[0]
        fr, er, carry, cbits = fs.frames_extract_numpy(np.packbits(seg), n, P, at % P, lock, carry, cbits, marker, m, d, pad)
        frames += list(fr)
        errors += list(er)
        locks += [(int(lock[0]), int(lock[1]))] * len(fr)
        at += n
    return np.array(frames, dtype=np.uint8).reshape(len(frames), (P - d + 7) // 8), np.array(errors, dtype=np.int64), locks
