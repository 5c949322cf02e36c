"""An independent restatement of the DAB+ superframe rules of include/vit_hip.h (vit_hip_dabplus_sync, vit_hip_dabplus_au_batch) on
plain Python integers and lists: one bit-serial shift register for both CRCs, the header read bit by bit.  It shares no code with
viterbidecodercpp_amd/dabplus.py, and the images it makes cover every element of every output buffer, written or not."""

EMPTY = (0, 0, 0xFFFFFFFF)
FORMATS = {(0, 1): (2, 5), (1, 1): (3, 6), (0, 0): (4, 8), (1, 0): (6, 11)}


def bit(data, t):
    return (data[t // 8] >> (7 - t % 8)) & 1


def shift_register(data, first_byte, n_bytes, poly, init):
    """the 16-bit register after the bits of data[first_byte : first_byte + n_bytes], the first transmitted bit first"""
    reg = init
    for t in range(8 * first_byte, 8 * (first_byte + n_bytes)):
        top = (reg >> 15) & 1
        reg = (reg << 1) & 0xFFFF
        if top ^ bit(data, t):
            reg ^= poly
    return reg


def fire_hit(frame):
    return shift_register(frame, 2, 9, 0x782F, 0) == frame[0] * 256 + frame[1] and any(frame[i] != 0 for i in range(11))


def au_crc(data, start, n):
    return shift_register(data, start, n, 0x1021, 0xFFFF) ^ 0xFFFF


def beats(ea, ca, eb, cb):
    return ca > 0 and (cb == 0 or ea * cb < eb * ca)


def sync_image(frames, counts, frame0, frame_bytes, hits=None, count=None):
    """frames [rows][F] of byte lists, counts [rows] or None, hits / count [rows][5] to add to or None.
    returns (hits [rows][5], count [rows][5], lock [rows][4])"""
    rows = len(frames)
    hits = [[0] * 5 for _ in range(rows)] if hits is None else [list(h) for h in hits]
    count = [[0] * 5 for _ in range(rows)] if count is None else [list(c) for c in count]
    lock = []
    for r in range(rows):
        nf = len(frames[r]) if counts is None else min(counts[r], len(frames[r]))
        for f in range(nf):
            p = (frame0 + f) % 5
            count[r][p] += 1
            hits[r][p] += 1 if fire_hit(frames[r][f]) else 0
        best = 0
        for p in range(1, 5):
            if beats(count[r][p] - hits[r][p], count[r][p], count[r][best] - hits[r][best], count[r][best]):
                best = p
        lock.append([best * 8 * frame_bytes, 0, count[r][best] - hits[r][best], count[r][best]])
    return hits, count, lock


def header(sf, s):
    """(fire_ok, consistent, n_aus, au_start [n_aus + 1], byte2) of one superframe (a byte list)"""
    dac, sbr = bit(sf, 17), bit(sf, 18)
    n_aus, first = FORMATS[(dac, sbr)]
    start = [first]
    for k in range(1, n_aus):
        v = 0
        for j in range(12):
            v = 2 * v + bit(sf, 24 + 12 * (k - 1) + j)
        start.append(v)
    start.append(110 * s)
    consistent = all(start[k + 1] >= start[k] + 3 for k in range(n_aus))
    return fire_hit(sf), consistent, n_aus, start, sf[2]


def au_image(superframes, counts, s, status, canary):
    """superframes [rows][F] of byte lists, counts [rows] or None, status [rows][F][s] or None.
    returns (info [rows * F], au [rows * F * 18]) with `canary` where nothing is written"""
    info, au = [], []
    for r, row in enumerate(superframes):
        nf = len(row) if counts is None else min(counts[r], len(row))
        for f, sf in enumerate(row):
            if f >= nf:
                info.append(canary)
                au += [canary] * 18
                continue
            fire_ok, consistent, n_aus, start, byte2 = header(sf, s)
            valid = fire_ok and consistent
            failed = status is not None and any(v < 0 for v in status[r][f])
            info.append(int(fire_ok) | int(consistent) << 1 | int(failed) << 2 | (n_aus if valid else 0) << 4 | byte2 << 8)
            for k in range(6):
                if valid and k < n_aus:
                    n = start[k + 1] - start[k] - 2
                    field = sf[start[k] + n] * 256 + sf[start[k] + n + 1]
                    au += [start[k], n, au_crc(sf, start[k], n) ^ field]
                else:
                    au += list(EMPTY)
    return info, au


def build_data(aus, dac, sbr, s, byte2_low=0, starts=None):
    """the 110 s data bytes of a superframe from access units (byte lists), bit by bit; `starts` overrides the header's au_start
    fields (hostile headers) without moving the access units"""
    n_aus, first = FORMATS[(dac, sbr)]
    assert len(aus) == n_aus
    data = [0] * (110 * s)
    data[2] = dac << 6 | sbr << 5 | (byte2_low & 31)
    at, where = first, []
    for a in aus:
        where.append(at)
        data[at:at + len(a)] = list(a)
        c = au_crc(data, at, len(a))
        data[at + len(a)], data[at + len(a) + 1] = c >> 8, c & 255
        at += len(a) + 2
    assert at == 110 * s, (at, 110 * s)
    fields = where[1:] if starts is None else list(starts)
    for k, v in enumerate(fields):
        for j in range(12):
            t = 24 + 12 * k + j
            data[t // 8] = (data[t // 8] & ~(1 << (7 - t % 8))) | ((v >> (11 - j)) & 1) << (7 - t % 8)
    c = shift_register(data, 2, 9, 0x782F, 0)
    data[0], data[1] = c >> 8, c & 255
    return data


def split_lengths(total, n, rng, fixed=()):
    """n access-unit lengths (each >= 1) whose bytes and CRCs fill `total`; `fixed` gives the first ones"""
    free = total - 2 * n - sum(fixed) - (n - len(fixed))
    assert free >= 0, (total, n, fixed)
    cuts = sorted(int(rng.integers(0, free + 1)) for _ in range(n - len(fixed) - 1))
    parts = [b - a for a, b in zip([0] + cuts, cuts + [free])] if n > len(fixed) else []
    return list(fixed) + [1 + p for p in parts]
