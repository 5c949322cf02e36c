"""An independent restatement of the DAB rules the package and the kernels are held to (ETSI EN 300 401 clauses 10, 11, 12), written for
the tests alone and sharing no code with viterbidecodercpp_amd/dab.py: the time de-interleaver as 16 per-residue FIFOs stepped frame by
frame, puncturing as a walk along the vectors symbol by symbol (the 24 vectors as a literal table), the energy-dispersal sequence as a
9-bit shift register clocked bit by bit -- and the images of the buffers one vit_hip_dab_deinterleave_batch or
vit_hip_dab_descramble_batch call leaves, sentinel included."""
import numpy as np

H = 15
POISON16, POISON8, POISON_BYTE = 0x5A5A, 0x5A, 0x5A
POISON_COUNT = 0x5A5A5A5A

PI = [None] + [v.replace(" ", "") for v in (
    "1100 1000 1000 1000 1000 1000 1000 1000",    # PI_1
    "1100 1000 1000 1000 1100 1000 1000 1000",    # PI_2
    "1100 1000 1100 1000 1100 1000 1000 1000",    # PI_3
    "1100 1000 1100 1000 1100 1000 1100 1000",    # PI_4
    "1100 1100 1100 1000 1100 1000 1100 1000",    # PI_5
    "1100 1100 1100 1000 1100 1100 1100 1000",    # PI_6
    "1100 1100 1100 1100 1100 1100 1100 1000",    # PI_7
    "1100 1100 1100 1100 1100 1100 1100 1100",    # PI_8
    "1110 1100 1100 1100 1100 1100 1100 1100",    # PI_9
    "1110 1100 1100 1100 1110 1100 1100 1100",    # PI_10
    "1110 1100 1110 1100 1110 1100 1100 1100",    # PI_11
    "1110 1100 1110 1100 1110 1100 1110 1100",    # PI_12
    "1110 1110 1110 1100 1110 1100 1110 1100",    # PI_13
    "1110 1110 1110 1100 1110 1110 1110 1100",    # PI_14
    "1110 1110 1110 1110 1110 1110 1110 1100",    # PI_15
    "1110 1110 1110 1110 1110 1110 1110 1110",    # PI_16
    "1111 1110 1110 1110 1110 1110 1110 1110",    # PI_17
    "1111 1110 1110 1110 1111 1110 1110 1110",    # PI_18
    "1111 1110 1111 1110 1111 1110 1110 1110",    # PI_19
    "1111 1110 1111 1110 1111 1110 1111 1110",    # PI_20
    "1111 1111 1111 1110 1111 1110 1111 1110",    # PI_21
    "1111 1111 1111 1110 1111 1111 1111 1110",    # PI_22
    "1111 1111 1111 1111 1111 1111 1111 1110",    # PI_23
    "1111 1111 1111 1111 1111 1111 1111 1111",    # PI_24
)]
TAIL = "110011001100110011001100"


def delay(j):
    """frames soft bit i = j mod 16 is sent late: j's four bits read backwards"""
    return int(format(j & 15, "04b")[::-1], 2)


def mask_walk(segments):
    """the puncturing mask of a profile, one entry per mother-code symbol, a list of 0 / 1"""
    out = []
    for blocks, pi in segments:
        for _ in range(blocks):
            for _ in range(4):
                for ch in PI[pi]:
                    out.append(int(ch))
    for ch in TAIL:
        out.append(int(ch))
    return out


def source_map(mask):
    idx, kept = [], 0
    for m in mask:
        idx.append(kept if m else -1)
        kept += 1 if m else 0
    return idx, kept


def puncture(codeword, mask):
    return [s for s, m in zip(codeword, mask) if m]


def depuncture(received, mask):
    it = iter(received)
    return [next(it) if m else 0 for m in mask]


def prbs_bits(n):
    reg = [1] * 9                                                  # reg[k] = p[t - 1 - k]
    out = []
    for _ in range(n):
        o = reg[4] ^ reg[8]
        out.append(o)
        reg = [o] + reg[:8]
    return out


def descramble_frame(frame, n_bits):
    """the ceil(n_bits / 8) bytes of a frame (a list of ints), its first n_bits bits XORed with the sequence"""
    nb = (n_bits + 7) // 8
    out = list(frame[:nb])
    for t, p in enumerate(prbs_bits(n_bits)):
        out[t // 8] ^= p << (7 - t % 8)
    return out


def fifo_deinterleave(S, n):
    """S: the frames of a row in order (sequences of n) -> the logical frames they complete, len(S) - 15 of them"""
    fifos = [[] for _ in range(16)]
    out = []
    for t, frame in enumerate(S):
        frame = list(frame)
        logical = [0] * n
        for j in range(16):
            fifos[j].append(frame[j::16])
            depth = H - delay(j)                                   # the receiver's delay of this residue
            if len(fifos[j]) > depth + 1:
                fifos[j].pop(0)
            if len(fifos[j]) == depth + 1:
                logical[j::16] = fifos[j][0]
        if t >= H:
            out.append(logical)
    return out


def deinterleave_image(frames, counts, hists, fills, n, max_frames, idx, poison):
    """what one call leaves.  frames[r]: max_frames frames of n; counts[r] / fills[r]: the uint32 values of the count memory (counts None:
    all; hists None: no history); hists[r]: 15 frames of n; idx: the map, a list (None: the identity).
    returns (out [rows * max_frames * spf], n_out [rows], hist_out [rows][15 n], fill_out [rows]), `poison` where nothing is written"""
    rows = len(frames)
    idx = list(range(n)) if idx is None else idx
    spf = len(idx)
    out, n_out, hist_out, fill_out = [], [], [], []
    for r in range(rows):
        nf = max_frames if counts is None else min(counts[r], max_frames)
        fill = 0 if hists is None else min(fills[r], H)
        S = [list(x) for x in hists[r][H - fill:]] if fill else []
        S += [list(frames[r][f]) for f in range(nf)]
        T = len(S)
        logical = fifo_deinterleave(S, n)
        assert len(logical) == max(0, T - H)
        n_out.append(len(logical))
        for k in range(max_frames):
            if k < len(logical):
                out += [logical[k][p] if 0 <= p < n else 0 for p in idx]
            else:
                out += [poison] * spf
        keep = min(H, T)
        row = [poison] * ((H - keep) * n)
        for s in S[T - keep:]:
            row += s
        hist_out.append(row)
        fill_out.append(keep)
    return out, n_out, hist_out, fill_out


def descramble_image(frames, counts, n_bits, max_frames, out_stride, poison=POISON_BYTE, before=None):
    """frames[r][f]: the bytes of a frame (at least ceil(n_bits / 8)) -> the out buffer [rows * max_frames * out_stride] one call leaves;
    before: what the buffer held (in place: the input itself), default all `poison`"""
    rows = len(frames)
    nb = (n_bits + 7) // 8
    out = [poison] * (rows * max_frames * out_stride) if before is None else list(before)
    for r in range(rows):
        nf = max_frames if counts is None else min(counts[r], max_frames)
        for f in range(nf):
            at = (r * max_frames + f) * out_stride
            out[at:at + nb] = descramble_frame(frames[r][f], n_bits)
    return out


def interleave(frames):
    """the transmit side, literally: b[r][i] = a[r - delay(i mod 16)][i], 0 in front of the first frame"""
    N, n = len(frames), len(frames[0])
    return [[frames[r - delay(i)][i] if r - delay(i) >= 0 else 0 for i in range(n)] for r in range(N)]


def pack_bits(bits):
    return np.packbits(np.asarray(bits, dtype=np.uint8))
