"""Rate of BatchDecoder.sync_search against the same hypotheses done as rounds of the existing calls, and of the build kernel against a
device-to-device copy of its output bytes.  Voyager K = 7 R = 1/2 SOFT16, unpunctured and under the 3/4 mask, H = 8 and 32
hypotheses, T = 48 + n 1024 + 48 for n = 16 and 64.  Timed with device events around work on one stream (the loop form ends every round
in a copy to the host, as a caller that ranks on the host does).

    python scripts/sync_search_rate.py [--out profiles/sync_search_rate.txt] [--reps 20]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MASK_3_4 = (1, 1, 0, 1, 1, 0)
QPSK = (0, 3, 6, 5)


def event_ms(torch, fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def gather_plan(torch, hyp, T, R, mask, device):
    """what a caller of the existing calls precomputes per hypothesis: the index, the erasures and the signs of its stream"""
    offset, flags = hyp
    if mask is None:
        source, kept = np.arange(R), R
    else:
        m = np.asarray(mask, dtype=bool)
        source, kept = np.where(m, np.cumsum(m) - 1, -1), int(m.sum())
    k = np.arange(T * R)
    s = source[k % source.size]
    live = s >= 0
    j = offset + (k // source.size) * kept + np.where(live, s, 0)
    jj = j ^ 1 if flags & 1 else j
    sign = np.where(np.where(j & 1, bool(flags & 4), bool(flags & 2)), -1, 1) * live
    return torch.from_numpy(jj).to(device), torch.from_numpy(sign.astype(np.int16)).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_search_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, get_decoding_config

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    code = COMMON_CODES[2]
    pc = get_decoding_config("SOFT16", code.R)
    table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
    R, W, head, tail, skip = code.R, 1024, 48, 48, 8
    lines = [f"# {torch.cuda.get_device_name(0)}; Voyager K=7 R=1/2 SOFT16, W={W}, head=tail={head}; ms per search of H hypotheses, device events, "
             f"{args.reps} repetitions after warm-up",
             "# mask  windows  T  H  one_call_ms  rounds_ms  ratio  build_ms  build_out_GB/s  build_moved_GB/s  copy_same_bytes_ms  copy_GB/s  build/copy"]
    for mask in (None, MASK_3_4):
        for windows in (16, 64):
            T = head + windows * W + tail
            for H in (8, 32):
                hyps = [(o, f) for o in range(H // 4) for f in QPSK]
                L = (T + 64) // 8 * 8 + 64
                _, sym = dec.synth(1, L, 4.0, seed=windows + H)
                flat = sym.reshape(-1)
                if mask is not None:
                    flat = flat[torch.from_numpy(np.resize(np.asarray(mask, dtype=bool), flat.numel())).cuda()]
                received = flat.contiguous()
                one = lambda: dec.sync_search(received, hyps, T, mask=mask, window=W, head=head, tail=tail)
                err, cmp, best = one()
                plans = [gather_plan(torch, h, T, R, mask, dec.device) for h in hyps]
                n_out = T - head - tail

                def rounds():
                    res = []
                    for idx, sign in plans:
                        stream = (received[idx] * sign).view(T, R)
                        out, n = dec.decode_stream(stream, begin=False, end=False, window=W, head=head, tail=tail)
                        state = (out[:1] & 63).to(torch.int32)
                        e, c = dec.channel_errors(stream[head + skip:head + n_out].reshape(1, -1), out[skip // 8:].view(1, -1), n_out - skip,
                                                  tail=False, start_state=state)
                        res.append((e.cpu(), c.cpu()))
                    return res

                res = rounds()
                assert [int(e) for e, _ in res] == err.cpu().tolist() and [int(c) for _, c in res] == cmp.cpu().tolist(), "the two forms disagree"
                for _ in range(2):
                    one(), rounds()
                one_ms = event_ms(torch, one, args.reps)
                rounds_ms = event_ms(torch, rounds, max(args.reps // 4, 2))
                pitch = (T + W - 1) // W * W
                built = torch.empty((H, pitch, R), dtype=torch.int16, device=dec.device)
                build = lambda: dec.sync_build(received, hyps, T, mask=mask, pitch=pitch, out=built)
                out_bytes = H * T * R * 2
                src = torch.empty(out_bytes, dtype=torch.uint8, device=dec.device)
                dst = torch.empty_like(src)
                copy = lambda: dst.copy_(src)
                for _ in range(3):
                    build(), copy()
                build_ms = event_ms(torch, build, 4 * args.reps)
                copy_ms = event_ms(torch, copy, 4 * args.reps)
                kept_share = 1.0 if mask is None else sum(mask) / len(mask)
                moved = out_bytes * (1 + kept_share)                      # written, and read from the received buffer (through the caches)
                lines.append(f"{'none' if mask is None else '3/4':>5} {windows:7d} {T:6d} {H:3d} {one_ms:10.4f} {rounds_ms:10.4f} {rounds_ms / one_ms:6.1f} "
                             f"{build_ms:9.5f} {out_bytes / build_ms / 1e6:9.1f} {moved / build_ms / 1e6:9.1f} {copy_ms:9.5f} {out_bytes / copy_ms / 1e6:9.1f} "
                             f"{copy_ms / build_ms:6.2f}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
