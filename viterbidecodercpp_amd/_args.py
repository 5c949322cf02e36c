"""The tensor rules of the Python host layer, each stated once: what decoder.py, outer.py and stream.py ask of a tensor before its address
goes to the C ABI.  Plain functions; each raises ValueError and names the argument (`what`).  Where the call sites once differed, the rule
is the more permissive of them, and says so."""
import numpy as np


def device(x, dtype, what):
    """a CUDA tensor of `dtype`: the part every rule shares; its layout is the caller's to check"""
    if x.dtype != dtype or not x.is_cuda:
        raise ValueError(f"{what} must be a {dtype} CUDA tensor")
    return x


def dense(x, dtype, numel, what):
    """a contiguous CUDA tensor of `dtype` with exactly `numel` elements (None: any number)"""
    if not device(x, dtype, what).is_contiguous() or (numel is not None and x.numel() != numel):
        raise ValueError(f"{what} must be a contiguous {dtype} CUDA tensor" + ("" if numel is None else f" of {numel} elements"))
    return x


def counts(x, rows, what):
    """None, or one int32 per row"""
    import torch
    return x if x is None else dense(x, torch.int32, rows, what)


def bit_rows(x, n_bits):
    """(rows, row stride) of `bytes`: uint8, one row or [rows][>= ceil(n_bits/8)] with contiguous rows.  An empty tensor may have any
    strides, and the stride of a single row is never used (0)"""
    import torch
    if device(x, torch.uint8, "bytes").dim() not in (1, 2) or (x.numel() and x.stride(-1) != 1):
        raise ValueError("bytes must be one row or [rows][>= ceil(n_bits/8)] with contiguous rows")
    if x.shape[-1] < (n_bits + 7) // 8:
        raise ValueError(f"{n_bits} bits need {(n_bits + 7) // 8} bytes per row of bytes")
    rows = 1 if x.dim() == 1 else int(x.shape[0])
    return rows, (int(x.stride(0)) if rows > 1 else 0)


def packets(x, what, least):
    """(rows, max_frames, packet stride) of a uint8 tensor [rows][max_frames][>= least] or [max_frames][...] (one row) with evenly spaced
    packets.  An empty tensor may have any strides; rows are only held to the spacing where there is more than one"""
    import torch
    if device(x, torch.uint8, what).dim() not in (2, 3) or (x.numel() and x.stride(-1) != 1) or x.shape[-1] < least:
        raise ValueError(f"{what} must be [rows][max_frames][>= {least}] or [max_frames][...] with contiguous packets")
    rows, mf = (1 if x.dim() == 2 else int(x.shape[0])), int(x.shape[-2])
    if x.dim() == 3 and rows > 1 and mf > 0 and x.stride(0) != mf * x.stride(1):
        raise ValueError(f"{what} must be evenly spaced")
    return rows, mf, (int(x.stride(-2)) if mf > 1 or rows > 1 else int(x.shape[-1]))


def row_buffer(x, rows, least, what, dtype=None):
    """the row stride of a buffer [rows][>= least] of `dtype` (None: uint8) with contiguous rows that is carried from call to call; a
    single row's stride is its width"""
    import torch
    if device(x, dtype or torch.uint8, what).dim() != 2 or x.shape[0] != rows or x.shape[1] < least or x.stride(1) != 1:
        raise ValueError(f"{what} must be [{rows}][>= {least}] with contiguous rows")
    return int(x.stride(0)) if rows > 1 else int(x.shape[1])


def carried(prev, prev_count, nxt, rows, least, what, counted, dtype=None):
    """the row stride of the row buffer `nxt` (`what`_out) a call writes and of `prev` (`what`), the one the call before wrote (None:
    nothing carried): `prev` comes with its int32 counts [rows] (`counted`), is another tensor than `nxt` and has its row stride"""
    stride = row_buffer(nxt, rows, least, f"{what}_out", dtype)
    if prev is not None:
        if counts(prev_count, rows, counted) is None:
            raise ValueError(f"{what} needs {counted}, an int32 tensor [{rows}]")
        if row_buffer(prev, rows, least, what, dtype) != stride or prev.data_ptr() == nxt.data_ptr():
            raise ValueError(f"{what} and {what}_out must be distinct tensors with the same row stride")
    return stride


def state_tensor(torch, device, states, frames=None, what="start_state"):
    """None, or the encoder / decoder states as a contiguous int32 tensor on `device`; with `frames`, flat and one per frame"""
    if states is None:
        return None
    states = torch.as_tensor(states, dtype=torch.int32, device=device)
    if frames is not None and states.numel() != frames:
        raise ValueError(f"{what} must hold one state per frame")
    return (states if frames is None else states.reshape(-1)).contiguous()


def puncture_map(owner, mask):
    """the int32 device tensor that names, per mother-code symbol of the boolean puncturing vector `mask`, the transmitted symbol it is
    (-1: punctured).  Built and uploaded once per puncturing scheme: `owner` (its .torch, .device) keeps the last one"""
    key = mask.tobytes()
    cached = getattr(owner, "_puncture_map", None)
    if cached is None or cached[0] != key:
        idx = np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int32)
        cached = owner._puncture_map = (key, owner.torch.from_numpy(idx).to(owner.device))
    return cached[1]


def lte_frames(received, dtype, D, E, offsets, counts):
    """(n_received, frames, frame stride, E_max) of an lte_rate_dematch call.  Without `offsets`, `received` is [frames][>= E] of `dtype`
    with contiguous rows (its row stride is the frame stride; one row: [>= E]) and E defaults to the row length; with `offsets`, int32 [F]
    (the uint32 values of the ABI), it is one contiguous region the offsets point into and E, the most one frame holds, must be given.
    `counts`: None, or int32 [frames].  The region ends with the tensor: nothing behind its last element is the call's to read"""
    import torch
    if not 1 <= int(D) <= 8192:
        raise ValueError("D must be 1 .. 8192")
    if offsets is not None:
        if E is None:
            raise ValueError("offsets need E, the most elements one frame holds")
        frames = dense(offsets, torch.int32, None, "offsets").numel()
        n, stride = dense(received, dtype, None, "received").numel(), 0
    else:
        if device(received, dtype, "received").dim() not in (1, 2) or (received.numel() and received.stride(-1) != 1):
            raise ValueError("received must be [frames][>= E] with contiguous rows (or one frame), or one region with offsets")
        E = int(received.shape[-1]) if E is None else int(E)
        if received.shape[-1] < E:
            raise ValueError(f"received holds {received.shape[-1]} elements per frame, E is {E}")
        frames = 1 if received.dim() == 1 else int(received.shape[0])
        stride = int(received.stride(0)) if frames > 1 else E
        if stride < E:
            raise ValueError("the frames of received overlap")
        n = (frames - 1) * stride + E if frames else 0
    E = int(E)
    if not 1 <= E < 1 << 24:
        raise ValueError("E must be 1 .. 2^24 - 1")
    if counts is not None:
        dense(counts, torch.int32, frames, "counts")
    return n, frames, stride, E


def soft_frames(x, dtype, what, least):
    """(rows, max_frames, row stride, frame stride), in elements, of a tensor of `dtype` [rows][max_frames][>= least] or [max_frames][...]
    (one row) whose frames are contiguous, do not overlap and lie in ascending order: a sub-channel cut out of whole CIFs as a view is
    read in place.  The strides of a single frame or row are never used (0: packed)"""
    if device(x, dtype, what).dim() not in (2, 3) or (x.numel() and x.stride(-1) != 1) or x.shape[-1] < least:
        raise ValueError(f"{what} must be [rows][max_frames][>= {least}] or [max_frames][...] with contiguous frames")
    rows, mf = (1 if x.dim() == 2 else int(x.shape[0])), int(x.shape[-2])
    fs = int(x.stride(-2)) if mf > 1 else 0
    rs = int(x.stride(0)) if x.dim() == 3 and rows > 1 else 0
    if (mf > 1 and fs < least) or (rows > 1 and rs < mf * (fs or least)):
        raise ValueError(f"the frames of {what} overlap")
    return rows, mf, rs, fs


def dabplus_frames(x, frame_bytes, frame0):
    """(rows, max_frames, row stride, frame stride), in bytes, of the logical frames of a dabplus_sync call: the rule of soft_frames on
    uint8, frame_bytes at least 11 and small enough for the lock's bit phase, frame0 one of the five places of a superframe"""
    import torch
    if not 11 <= frame_bytes <= 0x7FFFFFFF // 40:
        raise ValueError("frame_bytes must be 11 .. (2^31 - 1) / 40")
    if not 0 <= frame0 < 5:
        raise ValueError("frame0 must be 0 .. 4")
    return soft_frames(x, torch.uint8, "frames", frame_bytes)


def wifi_rows(x, dtype, least, what):
    """(frames, row stride in elements) of a tensor of `dtype` [frames][>= least] with contiguous rows, or one frame [>= least]: the soft
    bits of wifi_deinterleave, the decoded bytes of wifi_signal_parse and wifi_descramble.  Rows lie in ascending order and do not
    overlap.  The stride of a single row is its width: the ABI takes the bytes a call may read from the stride, and its own default (0)
    may be wider than the tensor"""
    if device(x, dtype, what).dim() not in (1, 2) or (x.numel() and x.stride(-1) != 1) or x.shape[-1] < least:
        raise ValueError(f"{what} must be [frames][>= {least}] of {dtype} with contiguous rows")
    frames = 1 if x.dim() == 1 else int(x.shape[0])
    stride = int(x.stride(0)) if frames > 1 else int(x.shape[-1])
    if frames > 1 and stride < least:
        raise ValueError(f"the frames of {what} overlap")
    return frames, stride


def wifi_soft(x, dtype, max_sym, S, rate, per_frame):
    """(frames, row stride) of the soft bits of a wifi_deinterleave call: the rule of wifi_rows with at least max_sym OFDM symbols a row,
    of N_CBPS(rate) soft bits each, or of 288 where the rate is per frame on the device.  max_sym and S at least 1, rate 0 .. 7"""
    from .wifi import WIFI_RATES
    if max_sym < 1 or S < 1 or not 0 <= rate <= 7:
        raise ValueError("max_sym and S must be at least 1, rate 0 .. 7")
    return wifi_rows(x, dtype, max_sym * (WIFI_RATES[7].n_cbps if per_frame else WIFI_RATES[rate].n_cbps), "soft")


def wifi_signal(x, frames, what="signal"):
    """the [frames][5] int32 tensor wifi_signal_parse returns -- (rate_index, length, n_sym, n_steps, valid), the uint32 values of the
    ABI --, dense: the per-frame arguments of the next stages point into it at an element stride of 5"""
    import torch
    if dense(x, torch.int32, frames * 5, what).dim() != 2 or x.shape[1] != 5:
        raise ValueError(f"{what} must be an int32 CUDA tensor [{frames}][5]")
    return x


def dvbt_symbols(x, dtype, cell):
    """(rows, n_sym, row stride in elements) of the soft bits of a dvbt_deinterleave call: a tensor of `dtype` [rows][n_sym][cell] or
    [n_sym][cell] (one row), cell = Nmax * v, whose rows are contiguous, lie in ascending order and do not overlap; a view with a larger
    row stride is read in place.  The stride of a single row is its length"""
    if device(x, dtype, "symbols").dim() not in (2, 3) or x.shape[-1] != cell:
        raise ValueError(f"symbols must be [rows][n_sym][{cell}] or [n_sym][{cell}] of {dtype}")
    rows, n_sym = (1 if x.dim() == 2 else int(x.shape[0])), int(x.shape[-2])
    if x.numel() and (x.stride(-1) != 1 or (n_sym > 1 and x.stride(-2) != cell)):
        raise ValueError("the OFDM symbols of a row of symbols must be contiguous")
    stride = int(x.stride(0)) if x.dim() == 3 and rows > 1 else n_sym * cell
    if stride < n_sym * cell:
        raise ValueError("the rows of symbols overlap")
    return rows, n_sym, stride


def dvbt_out(x, dtype, rows, steps):
    """the row stride in trellis steps of the output of a dvbt_deinterleave call: a tensor of `dtype` [rows][>= steps][2] (or [>= steps][2]
    with one row) with contiguous rows -- the [n_streams][pitch][R] buffer decode_streams reads, say"""
    if device(x, dtype, "out").dim() not in (2, 3) or x.shape[-1] != 2 or x.shape[-2] < steps or (1 if x.dim() == 2 else x.shape[0]) != rows:
        raise ValueError(f"out must be [{rows}][>= {steps}][2] of {dtype}")
    if x.numel() and (x.stride(-1) != 1 or (x.shape[-2] > 1 and x.stride(-2) != 2) or (x.dim() == 3 and rows > 1 and x.stride(0) % 2)):
        raise ValueError("the rows of out must be contiguous")
    if x.dim() == 3 and rows > 1 and x.stride(0) < 2 * steps:
        raise ValueError("the rows of out overlap")
    return int(x.stride(0)) // 2 if x.dim() == 3 and rows > 1 else int(x.shape[-2])


def is95_symbols(x, dtype, scramble):
    """(frames, row stride in elements, mask stride in bytes) of an is95_deinterleave call: symbols by the rule of wifi_rows with 384
    elements a frame; scramble None, a dense uint8 tensor [48] (stride 0: one mask for the batch) or [frames][>= 48] by that rule"""
    import torch
    frames, stride = wifi_rows(x, dtype, 384, "symbols")
    if scramble is None:
        return frames, stride, 0
    if scramble.dim() == 1:
        dense(scramble, torch.uint8, 48, "scramble")
        return frames, stride, 0
    sframes, sstride = wifi_rows(scramble, torch.uint8, 48, "scramble")
    if sframes != frames:
        raise ValueError(f"scramble must be [48] or [{frames}][>= 48]")
    return frames, stride, sstride


def is95_outputs(out, dtype, frames):
    """the four outputs of an is95_deinterleave call as a tuple: dense tensors of `dtype` with frames * 2 S_h elements, S_h = 192, 96, 48,
    24, or None where a hypothesis is not wanted -- not all four --, no two of which share storage"""
    out = tuple(out)
    if len(out) != 4 or all(x is None for x in out):
        raise ValueError("out must be four tensors, None where a hypothesis is not wanted, not all None")
    for h, x in enumerate(out):
        if x is not None:
            dense(x, dtype, frames * (384 >> h), f"out[{h}]")
    spans = sorted((x.data_ptr(), x.data_ptr() + x.numel() * x.element_size()) for x in out if x is not None and x.numel())
    if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        raise ValueError("the outputs must not share storage")
    return out


def is95_decoded(bytes, errors, compared, syndrome):
    """(frames, the four byte strides) of an is95_rate_decide call: bytes, four uint8 tensors by the rule of wifi_rows with 23, 11, 5 and 2
    bytes a frame in two dimensions, None for an absent hypothesis (stride 0), not all; for every present one dense int32 [frames] counts
    in errors and compared and, for the first two, in syndrome (errors None: the counts are not part of the call)"""
    import torch
    counted = errors is not None
    if len(bytes) != 4 or all(b is None for b in bytes) or (counted and (len(errors) != 4 or len(compared) != 4 or len(syndrome) < 2)):
        raise ValueError("bytes, errors and compared must hold four entries, syndrome two; not every hypothesis may be absent")
    frames, strides = None, []
    for h, b in enumerate(bytes):
        if b is None:
            strides.append(0)
            continue
        n, stride = wifi_rows(b, torch.uint8, (23, 11, 5, 2)[h], f"bytes[{h}]")
        if b.dim() != 2 or (frames is not None and n != frames):
            raise ValueError("every hypothesis must hold [frames] rows of bytes")
        frames = n
        strides.append(stride)
        for x, what in (((errors[h], "errors"), (compared[h], "compared")) + (((syndrome[h], "syndrome"),) if h < 2 else ())) if counted else ():
            if x is None:
                raise ValueError(f"{what}[{h}] is missing")
            dense(x, torch.int32, frames, f"{what}[{h}]")
    return frames, strides


def is95_counted(symbols, bytes, errors, compared, dtype, frames):
    """an is95_channel_errors call: for every hypothesis whose bytes are given, symbols[h] a dense tensor of `dtype` with frames * 2 S_h
    elements and errors[h], compared[h] dense int32 [frames], no two of the count tensors the same"""
    import torch
    if len(symbols) != 4 or len(errors) != 4 or len(compared) != 4:
        raise ValueError("symbols, errors and compared must hold four entries")
    seen = set()
    for h, b in enumerate(bytes):
        if b is None:
            continue
        if symbols[h] is None or errors[h] is None or compared[h] is None:
            raise ValueError(f"hypothesis {h} needs symbols, errors and compared")
        dense(symbols[h], dtype, frames * (384 >> h), f"symbols[{h}]")
        for x, what in ((errors[h], "errors"), (compared[h], "compared")):
            if dense(x, torch.int32, frames, f"{what}[{h}]").data_ptr() in seen and frames:
                raise ValueError("the count tensors must be distinct")
            seen.add(x.data_ptr())


def gsm_bursts(x, dtype):
    """(rows, bursts, row stride, burst stride), in elements, of a gsm_deinterleave call: the rule of soft_frames with 116 elements a
    burst, [rows][bursts][>= 116] or [bursts][...] (one row), bursts a multiple of 4"""
    rows, bursts, rs, bs = soft_frames(x, dtype, "bursts", 116)
    if bursts % 4:
        raise ValueError("bursts must hold a multiple of 4 bursts a row")
    return rows, bursts, rs, bs


def gsm_outputs(out, dtype, rows, blocks, diagonal):
    """the outputs of a gsm_deinterleave call, a dict: full, class1, class2 dense tensors of `dtype` with rows * blocks * 456 / 378 / 78
    elements, steal dense int32 [rows * blocks] -- not all four absent --, n_out int32 [rows]; in diagonal mode hist_out, dense of `dtype`
    with rows * 464 elements, together with fill_out, int32 [rows]; in block mode neither.  returns the seven in the ABI's order, None
    where absent"""
    import torch
    names = ("hist_out", "fill_out", "n_out", "full", "class1", "class2", "steal")
    if set(out) - set(names):
        raise ValueError(f"out may hold {names}")
    got = [out.get(k) for k in names]
    if all(x is None for x in got[3:]):
        raise ValueError("out must hold one of full, class1, class2, steal")
    if (got[0] is None) != (got[1] is None) or (not diagonal and got[0] is not None):
        raise ValueError("hist_out and fill_out come together, in diagonal mode only")
    for x, dt, n, k in zip(got, (dtype, torch.int32, torch.int32, dtype, dtype, dtype, torch.int32),
                           (rows * 464, rows, rows, rows * blocks * 456, rows * blocks * 378, rows * blocks * 78, rows * blocks), names):
        if x is not None:
            dense(x, dt, n, f"out[{k!r}]")
    return got
