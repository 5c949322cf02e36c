"""Tail-biting decoding restated on the CPU checker (oracle/viterbi_oracle.c), for the tail-biting tests.

The rule of vit_hip_decode_tail_biting_batch (include/vit_hip.h), written in terms of the reference's update / chainback:
extension ext[e] = symbols[(e - head) mod L] over S_ext = head + L + tail steps, every metric at initial_start_error, update()
over all of it, end state = argmin of the final metrics (unsigned error_t, lowest state on a tie), chainback over
L_ext = S_ext - (K-1) bits, output bits [head, head + L), flag = the path enters and leaves the window in the same state.
"""
import numpy as np

from viterbidecodercpp_amd import synth


def default_extension(K):
    return 8 * (K - 1)


def tb_reference(oracle, code, ocfg, sym, L, head=None, tail=None, want_metrics=False):
    """sym [F][L][R] soft -> (bytes [F][ceil(L/8)] uint8, end_state [F] uint32, ok [F] uint8), and with want_metrics the final
    metrics [F][N] uint32 the end state is chosen from"""
    K, R = code.K, code.R
    head = default_extension(K) if head is None else head
    tail = default_extension(K) if tail is None else tail
    sym = np.ascontiguousarray(sym).reshape(-1, L, R)
    F = sym.shape[0]
    S_ext = head + L + tail
    L_ext = S_ext - (K - 1)
    idx = (np.arange(S_ext) - head) % L
    table = oracle.branch_table(K, R, code.G, ocfg.high, ocfg.low)
    N = 1 << (K - 1)
    nb = (L + 7) // 8
    out = np.zeros((F, nb), dtype=np.uint8)
    ends = np.zeros(F, dtype=np.uint32)
    ok = np.zeros(F, dtype=np.uint8)
    final = np.zeros((F, N), dtype=np.uint32)
    for f in range(F):
        ext = np.ascontiguousarray(sym[f][idx])
        metrics = np.full(N, ocfg.initial_start_error, dtype=np.uint32)
        dec, _ = oracle.update(K, R, ocfg, table, metrics, ext)
        end = int(np.argmin(metrics))                      # first index of the minimum: the lowest state on a tie
        bits = np.unpackbits(oracle.chainback(K, dec, L_ext, end))[:L_ext]
        out[f] = np.packbits(bits[head:head + L], bitorder="big")[:nb]
        ends[f] = end
        ok[f] = 1 if np.array_equal(bits[head - K + 1:head], bits[head + L - K + 1:head + L]) else 0
        final[f] = metrics
    return (out, ends, ok, final) if want_metrics else (out, ends, ok)


def ml_tail_biting(code, sym, L):
    """exact maximum-likelihood tail-biting decoder: float64 correlation metrics, one Viterbi per start state constrained to start
    and end in it; returns the decoded info bits [F][L] uint8."""
    K, R, G = code.K, code.R, code.G
    N = 1 << (K - 1)
    sym = np.asarray(sym, dtype=np.float64).reshape(-1, L, R)
    F = sym.shape[0]
    ns = np.arange(N)
    b = ns & 1                                            # input bit of the branch into next state ns
    preds = np.stack([ns >> 1, (ns >> 1) | (N >> 1)])     # [2][N]: state = the last K-1 inputs, newest in bit 0
    # expected +-1 of every (predecessor choice, next state, polynomial): register = (pred << 1) | bit
    sign = np.zeros((2, N, R))
    for c in range(2):
        reg = (preds[c] << 1) | b
        for i in range(R):
            par = np.array([bin(int(x) & int(G[i])).count("1") & 1 for x in reg])
            sign[c, :, i] = 2.0 * par - 1.0
    best_metric = np.full(F, -np.inf)
    best_bits = np.zeros((F, L), dtype=np.uint8)
    for s0 in range(N):
        m = np.full((F, N), -np.inf)
        m[:, s0] = 0.0
        choice = np.zeros((L, F, N), dtype=np.uint8)
        for t in range(L):
            bm = np.einsum("fr,cnr->fcn", sym[:, t], sign)           # [F][2][N]
            cand = m[:, preds] + bm                                   # [F][2][N]
            c = (cand[:, 1] > cand[:, 0]).astype(np.uint8)
            choice[t] = c
            m = np.where(c == 1, cand[:, 1], cand[:, 0])
        fin = m[:, s0]
        better = fin > best_metric
        if not better.any():
            continue
        st = np.full(F, s0)
        bits = np.zeros((F, L), dtype=np.uint8)
        for t in range(L - 1, -1, -1):
            bits[:, t] = st & 1
            c = choice[t, np.arange(F), st]
            st = preds[c, st]
        best_metric = np.where(better, fin, best_metric)
        best_bits[better] = bits[better]
    return best_bits


def tb_frames(code, pc, F, L, ebn0, seed):
    """(info bits [F][L], symbols [F][L][R]) of random tail-biting codewords through the AWGN quantiser; ebn0 None: noise-free"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=(F, L), dtype=np.uint8)
    coded = synth.encode_tail_biting_numpy(code.K, code.R, code.G, bits)
    sym = synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, ebn0, code.R, rng, pc.soft_dtype)
    return bits, sym
