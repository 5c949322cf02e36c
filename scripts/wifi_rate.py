"""Time of the three 802.11a/g kernels -- BatchDecoder.wifi_deinterleave on the DATA field, wifi_signal_parse, wifi_descramble -- each
against three things in the same run:
  (a) copy: a device-to-device copy of as many bytes as the call reads plus writes;
  (b) decode: the decode call behind it (de-interleave: the DATA decode on the symbols it wrote) or in front of it (parse: the SIGNAL
      decode, L = 18; descramble: the DATA decode);
  (c) torch: the same result from torch index / bit ops on the device, what a caller does without the call, checked equal to the
      kernel's output before it is timed: per rate one index_select through a zero column (the padded input is built once, outside the
      timed call) and a mask of the steps; the SIGNAL fields by one broadcast shift, two sums and a 16-entry table; the descrambling by a [128][bytes] sequence table, an XOR and a 256-entry bit-reversal table.  The
      torch descrambler does NOT compute the FCS (a CRC has no torch op): its column flatters torch.
Shapes: 4096 PPDUs of 1500 octets at 54 Mbit/s (56 OFDM symbols), and 4096 of mixed rate and length in buffers of the same size.
The soft bits and decoded bytes are random: the kernels' work does not depend on the values.
Every figure is the median of `--sets` windows of `--reps` calls between two device events, after warm-up.

    python scripts/wifi_rate.py [--out profiles/wifi_rate.txt] [--reps 20] [--sets 7]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(torch, fn, reps, sets):
    times = []
    for _ in range(sets):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / reps)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wifi_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    ap.add_argument("--frames", type=int, default=4096)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (WIFI_POLYNOMIALS, WIFI_RATES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, get_decoding_config,
                                       wifi_scrambler_numpy)
    from viterbidecodercpp_amd.wifi import _source_index

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    pc = get_decoding_config("SOFT16", 2)
    dec = BatchDecoder(ViterbiBranchTable(7, 2, WIFI_POLYNOMIALS, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype),
                       ViterbiDecoder_Config.from_decoder_config(pc))
    dev = dec.device
    rng = np.random.default_rng(1)
    F = args.frames
    max_sym = -(-(22 + 8 * 1500) // 216)
    S, nb = max_sym * 216, (max_sym * 216 - 6 + 7) // 8
    max_length = (S - 22) // 8
    lines = [f"# {torch.cuda.get_device_name(0)}; the 802.11a/g kernels, SOFT16, {F} PPDUs in buffers of {max_sym} OFDM symbols (S = {S}); ms per call, "
             f"device events, median of {args.sets} windows of {args.reps} calls after warm-up; copy = device-to-device copy of the bytes read plus "
             "written; decode = the decode call beside it; torch = the same result from torch ops (the descrambler's without the FCS)",
             "# shape  call  kernel_ms  GB/s  copy_ms  kernel/copy  decode_ms  kernel/decode  torch_ms  torch/kernel"]

    soft = torch.from_numpy(rng.integers(-127, 128, size=(F, max_sym * 288)).astype(np.int16)).to(dev)
    padded = torch.cat([soft, soft.new_zeros((F, 1))], dim=1)                           # the torch ops' input: a zero column behind, built once
    sig_soft = torch.from_numpy(rng.integers(-127, 128, size=(F, 24, 2)).astype(np.int16)).to(dev)
    dbytes = torch.from_numpy(rng.integers(0, 256, size=(F, nb), dtype=np.uint8)).to(dev)
    sig_bytes = torch.from_numpy(rng.integers(0, 256, size=(F, 3), dtype=np.uint8)).to(dev)
    sym = torch.empty((F, S, 2), dtype=torch.int16, device=dev)
    psdu = torch.empty((F, max_length), dtype=torch.uint8, device=dev)
    status = torch.empty((F, 4), dtype=torch.int32, device=dev)
    parsed = torch.empty((F, 5), dtype=torch.int32, device=dev)
    decoded, sig_decoded = torch.empty((F, nb), dtype=torch.uint8, device=dev), torch.empty((F, 3), dtype=torch.uint8, device=dev)
    seq_table = torch.from_numpy(np.stack([np.packbits(wifi_scrambler_numpy(s, 8 * nb)) for s in range(128)])).to(dev)
    rev_table = torch.from_numpy(np.array([int(format(b, "08b")[::-1], 2) for b in range(256)], dtype=np.uint8)).to(dev)
    rate_table = torch.tensor([8, 6, 8, 7, 8, 2, 8, 3, 8, 4, 8, 5, 8, 0, 8, 1], dtype=torch.int32, device=dev)
    bit_shift = torch.arange(23, 5, -1, dtype=torch.int32, device=dev)[None, :]
    length_weight = (1 << torch.arange(12, dtype=torch.int32, device=dev))[None, :]
    ndbps = torch.tensor([r.n_dbps for r in WIFI_RATES] + [1], dtype=torch.int32, device=dev)

    def row(shape, call, n_bytes, kernel, decode, torch_fn, same):
        buf = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)
        copy = lambda: dst.copy_(buf)                                                  # noqa: E731
        for _ in range(3):
            kernel(), copy(), decode(), torch_fn()
        kernel()
        assert same(torch_fn()), f"{shape} {call}: the torch ops and the kernel differ"
        t = [median_ms(torch, fn, args.reps, args.sets) for fn in (kernel, copy, decode, torch_fn)]
        lines.append(f"{shape:>6s} {call:>12s} {t[0]:10.5f} {n_bytes / t[0] / 1e6:9.1f} {t[1]:10.5f} {t[0] / t[1]:7.2f} {t[2]:10.5f} {t[0] / t[2]:8.4f} "
                     f"{t[3]:10.5f} {t[3] / t[0]:8.2f}")
        print(lines[-1], flush=True)

    for shape in ("54", "mixed"):
        if shape == "54":
            rates, lengths = np.full(F, 7), np.full(F, 1500)
        else:
            rates = np.arange(F) % 8
            lengths = np.array([1 + rng.integers(0, (max_sym * WIFI_RATES[m].n_dbps - 22) // 8) for m in rates])
        n_steps = 22 + 8 * lengths
        n_sym = -(-n_steps // np.array([WIFI_RATES[m].n_dbps for m in rates]))
        signal = torch.from_numpy(np.stack([rates, lengths, n_sym, n_steps, np.ones(F)], axis=1).astype(np.int32)).to(dev)
        d_steps = signal[:, 3].contiguous()
        read = int((n_sym * np.array([WIFI_RATES[m].n_cbps for m in rates])).sum())           # soft bits of the frames' own symbols
        groups = []
        for m in sorted(set(rates.tolist())):
            src = _source_index(m, max_sym * WIFI_RATES[m].n_dbps)
            idx = np.full(2 * S, max_sym * 288, dtype=np.int64)                        # the zero column
            idx[:src.size] = np.where(src >= 0, src, max_sym * 288)
            groups.append((torch.from_numpy(np.flatnonzero(rates == m)).to(dev), torch.from_numpy(idx).to(dev)))
        step_of = (torch.arange(2 * S, device=dev) // 2)[None, :]
        ref_sym = torch.empty((F, 2 * S), dtype=torch.int16, device=dev)

        def deint_torch():
            for sel, idx in groups:
                ref_sym[sel] = padded[sel].index_select(1, idx) if len(groups) > 1 else padded.index_select(1, idx)
            return ref_sym.masked_fill_(step_of >= d_steps[:, None], 0)

        row(shape, "deinterleave", read * 2 + 12 * F + sym.numel() * 2, lambda: dec.wifi_deinterleave(soft, max_sym, S, signal=signal, out=sym),
            lambda: dec.decode(sym, S - 6, out=decoded), deint_torch, lambda r: torch.equal(r.view(-1), sym.view(-1)))

        def descramble_torch():
            seed = (dbytes[:, 0] >> 1).to(torch.int64)
            clear = dbytes ^ seq_table[seed]
            return rev_table[clear[:, 2:2 + max_length].to(torch.int64)]

        def same_psdu(r):
            keep = torch.arange(max_length, device=dev)[None, :] < signal[:, 1:2]
            return torch.equal(torch.where(keep, r, 0), torch.where(keep, psdu, 0))

        row(shape, "descramble", int(lengths.sum()) * 2 + 2 * F + 4 * F + 16 * F,
            lambda: dec.wifi_descramble(dbytes, S, signal, max_length=max_length, out=(psdu, status)), lambda: dec.decode(sym, S - 6, out=decoded),
            descramble_torch, same_psdu)

    def parse_torch():
        b = sig_bytes.to(torch.int32)
        w = b[:, 0] << 16 | b[:, 1] << 8 | b[:, 2]
        rate = rate_table[(w >> 20).to(torch.int64)]
        bits = (w[:, None] >> bit_shift) & 1                                             # [F][18], decoded bit t in column t
        length = (bits[:, 5:17] * length_weight).sum(dim=1, dtype=torch.int32)
        ones = bits.sum(dim=1, dtype=torch.int32)
        valid = ((rate < 8) & (ones % 2 == 0) & (((w >> 19) & 1) == 0) & (length >= 1)).to(torch.int32)
        steps = valid * (22 + 8 * length)
        per = ndbps[torch.where(valid == 1, rate, 8).to(torch.int64)]
        return torch.stack([rate, length, (steps + per - 1) // per, steps, valid], dim=1)

    row("signal", "parse", 3 * F + 20 * F, lambda: dec.wifi_signal_parse(sig_bytes, out=parsed), lambda: dec.decode(sig_soft, 18, out=sig_decoded), parse_torch,
        lambda r: torch.equal(r, parsed))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
