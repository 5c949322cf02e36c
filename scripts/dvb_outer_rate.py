"""Time of one BatchDecoder.deinterleave and one BatchDecoder.dvb_derandomize against a device-to-device copy of the same bytes, against
the rs_decode between them and against the frames_extract and decode_stream(s) calls in front, in one run.  DVB-S behind Voyager K = 7 R =
1/2 SOFT16: the (12, 17) interleaver, RS(204,188) and the energy dispersal on the 204-byte packets of one stream of 2^26 bits at P =
1632, and on 64 rows of 16384 bits.  The stream is clean (the calls' times do not depend on the data, but for rs_decode, which is timed
on words without errors).  dvb_derandomize is timed out of place with the phase known, out of place with the phase voted (every block of
a row reads all of the row's sync bytes) and in place (one workgroup per row).  Every figure is the median of `--sets` windows of
`--reps` calls between two device events, after warm-up; the decode_stream(s) baseline is the median of 3 windows of reps / 4 calls.

    python scripts/dvb_outer_rate.py [--out profiles/dvb_outer_rate.txt] [--reps 20] [--sets 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvb_outer_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (COMMON_CODES, DVB_INTERLEAVER, DVB_RS_204_188, DVB_SYNC, BatchDecoder, ViterbiBranchTable,
                                       ViterbiDecoder_Config, conv_interleave_numpy, dvb_randomize_numpy, get_decoding_config, rs_encode_numpy)

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    conv = COMMON_CODES[2]
    pc = get_decoding_config("SOFT16", conv.R)
    table = ViterbiBranchTable(conv.K, conv.R, conv.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
    (B, M), rs, P, W, n, H = DVB_INTERLEAVER, DVB_RS_204_188, 1632, 1024, 204, 11
    rng = np.random.default_rng(1)
    lines = [f"# {torch.cuda.get_device_name(0)}; DVB-S outer chain behind Voyager K=7 R=1/2 SOFT16 decoded at window {W}: interleaver (12,17), "
             f"RS(204,188), energy dispersal; ms per call, device events, median of {args.sets} windows of {args.reps} calls after warm-up "
             f"(decode_ms: 3 windows of {max(args.reps // 4, 2)}); copy = device-to-device copy of the rows x packets x 204 bytes",
             "# rows  packets/row  MB  copy_ms  deint_ms  deint/copy  deint_GB/s  derand_ms  derand/copy  derand_voted_ms  derand_inplace_ms  "
             "rs_clean_ms  extract_ms  decode_ms  (deint+derand)/decode"]
    for rows, per_row in ((1, (1 << 26) // P), (64, 16384 // P)):
        # a stream with a period of 96 packets: interleaved, it is periodic too behind its first H packets, and de-interleaves to valid words
        ts = rng.integers(0, 256, size=(96, 188), dtype=np.uint8)
        ts[:, 0] = 0x47
        words = rs_encode_numpy(rs, dvb_randomize_numpy(ts), 1)
        sent = conv_interleave_numpy(np.tile(words, (-(-(per_row + 96) // 96), 1)), B, M)[96:96 + per_row]
        bits = np.broadcast_to(np.unpackbits(sent.reshape(-1)), (rows, per_row * P))
        n_bits = bits.shape[1]
        d_info = torch.from_numpy(np.packbits(bits, axis=1)).to(dec.device)
        sym = dec.encode(d_info, n_bits, tail=True)
        if rows == 1:
            decode = lambda: dec.decode_stream(sym[0], begin=True, end=True, window=W)
        else:
            pitch = -(-sym.shape[1] // W) * W
            padded = torch.zeros((rows, pitch, conv.R), dtype=sym.dtype, device=sym.device)
            padded[:, :sym.shape[1]] = sym
            decode = lambda: dec.decode_streams(padded, sym.shape[1], begin=True, end=True, window=W)
        out, got_bits = decode()
        assert got_bits == n_bits
        lock = torch.zeros((rows, 4), dtype=torch.int32, device=dec.device)                      # the packets start at bit 0
        ex = dec.frames_extract(out, n_bits, P, 0, lock, marker=DVB_SYNC[0], marker_bits=8)
        extract = lambda: dec.frames_extract(out, n_bits, P, 0, lock, marker=DVB_SYNC[0], marker_bits=8, out=ex)
        packets, counts = ex[0], ex[1]
        assert int(counts.min().item()) == per_row and np.array_equal(packets[0].cpu().numpy(), sent)
        # the H packets in front of the stream's first as history, so that every input packet gives an output packet
        before = conv_interleave_numpy(np.tile(words, (2, 1)), B, M)[96 - H:96]
        hist = torch.from_numpy(np.broadcast_to(before.reshape(1, -1), (rows, H * n)).copy()).to(dec.device)
        fill = torch.full((rows,), H, dtype=torch.int32, device=dec.device)
        de = dec.deinterleave(packets, counts, B, M, hist, fill)
        deint = lambda: dec.deinterleave(packets, counts, B, M, hist, fill, out=de)
        status = torch.empty((rows, per_row, 1), dtype=torch.int32, device=dec.device)
        rs_clean = lambda: dec.rs_decode(rs, de[0], de[1], 1, status=status)
        rs_clean()
        assert int(de[1].min().item()) == per_row and not status.any().item()
        # the output lags the input by H packets: its packet 0 is packet 96 - H = 85 of the periodic stream, the sixth of its group
        phase = torch.full((rows,), (96 - H) % 8, dtype=torch.int32, device=dec.device)
        dr = dec.dvb_derandomize(de[0], de[1], phase, status)
        first = min(96, per_row)
        assert np.array_equal(dr[0][0, :first].cpu().numpy(), np.roll(ts, -(96 - H), axis=0)[:first]) and not dr[2].any().item()
        derand = lambda: dec.dvb_derandomize(de[0], de[1], phase, status, out=dr[0], phase_out=dr[1], sync_errors=dr[2])
        voted = lambda: dec.dvb_derandomize(de[0], de[1], None, status, out=dr[0], phase_out=dr[1], sync_errors=dr[2])
        work = de[0].clone()
        inplace = lambda: dec.dvb_derandomize(work, de[1], phase, status, phase_out=dr[1], sync_errors=dr[2], in_place=True)
        dst = torch.empty_like(packets)
        copy = lambda: dst.copy_(packets)
        for fn in (copy, deint, rs_clean, derand, voted, inplace, extract, decode):
            for _ in range(3):
                fn()
        copy_ms, deint_ms, rs_ms, derand_ms, voted_ms, inplace_ms, extract_ms = (median_ms(torch, fn, args.reps, args.sets)
                                                                                 for fn in (copy, deint, rs_clean, derand, voted, inplace, extract))
        decode_ms = median_ms(torch, decode, max(args.reps // 4, 2), 3)
        lines.append(f"{rows:6d} {per_row:7d} {packets.numel() / 1e6:8.3f} {copy_ms:9.5f} {deint_ms:9.5f} {deint_ms / copy_ms:7.2f} "
                     f"{packets.numel() / deint_ms / 1e6:9.1f} {derand_ms:9.5f} {derand_ms / copy_ms:7.2f} {voted_ms:9.5f} {inplace_ms:9.5f} "
                     f"{rs_ms:9.5f} {extract_ms:9.5f} {decode_ms:9.4f} {(deint_ms + derand_ms) / decode_ms:8.4f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
