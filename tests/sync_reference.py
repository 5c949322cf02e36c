"""Node synchronisation restated on the CPU, for the sync tests: the stream of a hypothesis (the bit-exact rule of vit_hip_sync_build,
include/vit_hip.h), the search by composition (stream_reference.stream_reference with flags = 0, a shift-register encoder from a start
state, synth.channel_errors_numpy), the ranking, and the channel that makes the test inputs.  The cases both test files use are built
once per process (CASES / make_case / case_reference).
"""
import functools

import numpy as np

from viterbidecodercpp_amd import COMMON_CODES, get_decoding_config, synth
from viterbidecodercpp_amd.codes import Code
from viterbidecodercpp_amd.sync import NEG_EVEN, NEG_ODD, SWAP, enumerate_hypotheses
from tests import stream_reference as sr
from tests.helpers import oracle_cfg

MAX_HYPOTHESES = 64
SHAPE_EBN0 = 6.0        # the extensions-and-windows cases: short heads and tails decode poorly, the truth must still win


def source_map(mask):
    """(source_index [period] int32, kept_per_period) of a 0/1 puncturing mask over one period: what BatchDecoder.depuncture builds"""
    mask = np.asarray(mask).astype(bool).reshape(-1)
    return np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int32), int(mask.sum())


def _scheme(R, mask):
    if mask is None:
        return np.arange(R, dtype=np.int32), R
    return source_map(mask)


def needed_received(hypotheses, T, R, mask=None):
    """the host-side bound of the C ABI: received symbols the call demands (the largest jj it allows itself to read, plus one).  Whole
    periods read all their kept symbols; a last partial one counts exactly without a map, as a whole one with a map"""
    source, kept = _scheme(R, mask)
    full, rem = divmod(T * R, source.size)
    span = full * kept + (0 if rem == 0 else kept if mask is not None else rem)
    need = 0
    for offset, flags in hypotheses:
        last = offset + span - 1
        if flags & SWAP:
            last |= 1
        need = max(need, last + 1)
    return need


def build_stream(received, offset, flags, T, R, high, low, mask=None):
    """the [T][R] stream of hypothesis (offset, flags): output symbol k reads received[jj], jj = j ^ 1 under SWAP, j = offset +
    (k // period) * kept + source[k % period]; erasure 0 where source < 0; mirrored about (high + low) / 2 and clamped to the type
    where the negate flag for the parity of j is set"""
    received = np.asarray(received)
    source, kept = _scheme(R, mask)
    info = np.iinfo(received.dtype)
    k = np.arange(T * R, dtype=np.int64)
    s = source[k % source.size].astype(np.int64)
    live = (s >= 0) & (s < kept)
    j = offset + (k // source.size) * kept + np.where(live, s, 0)
    jj = j ^ 1 if flags & SWAP else j
    if jj[live].max(initial=-1) >= received.size:
        raise IndexError("the hypothesis reads past the received buffer")
    v = received[np.where(live, jj, 0)].astype(np.int64)
    negate = np.where(j & 1, bool(flags & NEG_ODD), bool(flags & NEG_EVEN))
    v = np.where(negate, np.clip(high + low - v, info.min, info.max), v)
    return np.where(live, v, 0).astype(received.dtype).reshape(T, R)


def impair(sent, offset, flags, high, low, rng, pad=2):
    """the channel whose inverse hypothesis (offset, flags) is: `sent` (the transmitted symbols, 1-D, the first one the first symbol
    of a puncturing period) behind `offset` symbols of noise, I and Q swapped / mirrored so that build_stream(.., offset, flags) reads
    `sent` back; `pad` noise symbols behind (a swap moves the last symbol one further)"""
    sent = np.asarray(sent)
    rec = rng.integers(low, high + 1, size=offset + sent.size + pad).astype(sent.dtype)
    j = offset + np.arange(sent.size, dtype=np.int64)
    negate = np.where(j & 1, bool(flags & NEG_ODD), bool(flags & NEG_EVEN))
    rec[j ^ 1 if flags & SWAP else j] = np.where(negate, high + low - sent.astype(np.int64), sent).astype(sent.dtype)
    return rec


def skip_bits(K):
    return 8 * ((K - 1 + 7) // 8)


def encode_from_state(code, bits, state):
    """shift-register encoder from a start state in the decoder's numbering (bit j = the input j+1 steps back): bits [L] -> coded
    bits [L][R]"""
    out = np.zeros((len(bits), code.R), dtype=np.uint8)
    reg_mask = (1 << code.K) - 1
    reg = int(state)
    for t, b in enumerate(bits):
        reg = ((reg << 1) | int(b)) & reg_mask
        for i, g in enumerate(code.G):
            out[t, i] = bin(reg & int(g)).count("1") & 1
    return out


def beats(ea, ca, eb, cb):
    return ca > 0 and (cb == 0 or int(ea) * int(cb) < int(eb) * int(ca))


def rank(errors, compared):
    """the lowest index no other hypothesis beats"""
    n = len(errors)
    for i in range(n):
        if not any(beats(errors[j], compared[j], errors[i], compared[i]) for j in range(n) if j != i):
            return i
    raise AssertionError("the relation orders the rates: somebody is unbeaten")


def low32_misordered(ea, ca, eb, cb):
    """a beats b, and a comparison of the products' low 32 bits would not say so"""
    low = 0xFFFFFFFF
    return beats(ea, ca, eb, cb) and not (ea * cb) & low < (eb * ca) & low


def _first_misordered(pairs):
    return next(p for p in pairs if low32_misordered(*p))


# rates near 3e9 / 4e9 against a neighbour one count away: the 64-bit products differ by less than 2^32, and their low halves order
# the other way (one more error: the first such e from 3e9 up; one more compared: likewise) or are equal (1.5e9 of 2^31 compared, two errors
# apart: the products differ by exactly 2^32).  (e_a, c_a, e_b, c_b), a the better
WRAP_MORE_ERRORS = _first_misordered((e, 4_000_000_000, e + 1, 4_000_000_000) for e in range(3_000_000_000, 3_000_000_064))
WRAP_FEWER_COMPARED = _first_misordered((e, 4_000_000_000, e, 3_999_999_999) for e in range(3_000_000_000, 3_000_000_064))
WRAP_EQUAL_LOW = (1_500_000_000, 1 << 31, 1_500_000_002, 1 << 31)

# the hand-written inputs of the ranking, for rank() here (tests/test_sync_cpu.py pins the winners) and for sync_pick_kernel
# (tests/test_gpu_sync_kernels.py): name, errors, compared, the winner
RANK_SETS = [
    ("equal rates, other denominators", [3, 1, 5, 2, 7, 3], [4, 2, 8, 4, 9, 6], 1),                # 1/2, 2/4 and 3/6 at 1, 3 and 5
    ("equal rates behind a worse one", [2, 3, 2, 1], [3, 6, 4, 2], 1),                              # 3/6, 2/4, 1/2 at 1, 2 and 3
    ("errors = compared everywhere", [7, 3, 9, 1, 64], [7, 3, 9, 1, 64], 0),
    ("no errors, other compared", [0, 0, 0], [5, 9, 2], 0),
    ("no errors behind a live one", [4, 0, 0, 0], [8, 5, 9, 2], 1),
    ("nothing compared at index 0", [0, 9, 3, 4], [0, 10, 10, 10], 2),
    ("nothing compared anywhere", [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], 0),
    ("one more error, low halves the other way", [WRAP_MORE_ERRORS[2], WRAP_MORE_ERRORS[0]], [WRAP_MORE_ERRORS[3], WRAP_MORE_ERRORS[1]], 1),
    ("one compared fewer, low halves the other way", [WRAP_FEWER_COMPARED[2], WRAP_FEWER_COMPARED[0]],
     [WRAP_FEWER_COMPARED[3], WRAP_FEWER_COMPARED[1]], 1),
    ("products 2^32 apart", [WRAP_EQUAL_LOW[2], WRAP_EQUAL_LOW[0]], [WRAP_EQUAL_LOW[3], WRAP_EQUAL_LOW[1]], 1),
    ("one hypothesis", [3], [7], 0),
    ("one hypothesis, nothing compared", [0], [0], 0),
    ("63, the winner last", [10] * 62 + [9], [100] * 63, 62),
    ("64, the winner last", [10] * 63 + [9], [100] * 64, 63),
    ("64, the winner last by one in 2^32", [0xFFFFFFFE] * 63 + [0xFFFFFFFD], [0xFFFFFFFF] * 64, 63),
]


RANDOM_RANK_SEED, RANDOM_RANK_SETS = 2024, 2000


@functools.lru_cache(maxsize=None)
def random_rank_sets(seed=RANDOM_RANK_SEED, count=RANDOM_RANK_SETS):
    """[(errors, compared)] uint32: n uniform in 1 .. 64; the even sets draw errors <= compared from 0 .. 6, where ties for first
    place are common, the odd ones from the whole 32-bit range"""
    rng = np.random.default_rng(seed)
    sets = []
    for s in range(count):
        n = int(rng.integers(1, MAX_HYPOTHESES + 1))
        top = 6 if s % 2 == 0 else 0xFFFFFFFF
        a, b = rng.integers(0, top + 1, size=(2, n), dtype=np.uint64)
        sets.append((np.minimum(a, b).astype(np.uint32), np.maximum(a, b).astype(np.uint32)))
    return sets


def tied_for_first(errors, compared):
    """how many hypotheses have the winner's rate"""
    e, c = [int(x) for x in errors], [int(x) for x in compared]
    w = rank(e, c)
    if c[w] == 0:
        return len(c)                       # nothing compared anywhere: nobody beats anybody
    return sum(1 for i in range(len(e)) if c[i] > 0 and e[i] * c[w] == e[w] * c[i])


def search_reference(oracle, code, decode_type, received, hypotheses, T, W, head, tail, mask=None):
    """(errors [H], compared [H], best, decoded bits per hypothesis) by composition: build, stream_reference with flags = 0, the
    start state from the first skip bits, the rest re-encoded and counted against the hypothesis's own symbols"""
    pc = get_decoding_config(decode_type, code.R)
    high, low = pc.soft_decision_high, pc.soft_decision_low
    ocfg = oracle_cfg(decode_type, code.R)
    skip = skip_bits(code.K)
    errors, compared, decoded = [], [], []
    for offset, flags in hypotheses:
        stream = build_stream(received, offset, flags, T, code.R, high, low, mask)
        by, n = sr.stream_reference(oracle, code, ocfg, stream, W, head, tail, flags=0)
        assert n == T - head - tail and n > skip
        bits = np.unpackbits(by)[:n]
        state = sum(int(bits[skip - 1 - j]) << j for j in range(code.K - 1))
        coded = encode_from_state(code, bits[skip:], state)
        e, c = synth.channel_errors_numpy(code, high, low, stream[None, head + skip:head + n], coded[None])
        errors.append(int(e[0]))
        compared.append(int(c[0]))
        decoded.append(bits)
    return np.asarray(errors, dtype=np.int64), np.asarray(compared, dtype=np.int64), rank(errors, compared), decoded


def is_transparent(code):
    """every polynomial of odd weight: the complement of a codeword is a codeword"""
    return all(bin(int(g)).count("1") & 1 for g in code.G)


def equivalent(code, a, b):
    """hypotheses the count cannot tell apart: the same, or -- on a transparent code -- each other's inversion"""
    return a == b or (is_transparent(code) and a[0] == b[0] and a[1] ^ b[1] == (NEG_EVEN | NEG_ODD))


def aligned(case, hypothesis):
    """equivalent to the truth of a case (make_case), a whole number of periods later: an offset beyond one period reads the same
    stream further on"""
    kept = case["code"].R if case["mask"] is None else int(case["mask"].sum())
    return equivalent(case["code"], (hypothesis[0] % kept, hypothesis[1]), case["truth"])


# ---- the cases of tests/test_sync_cpu.py and tests/test_gpu_sync_search.py ----------------------------------------------------

K5, VOYAGER, LTE, DAB, IS95, CASSINI = 1, 2, 3, 4, 5, 7
K11 = Code("K11R2", 11, 2, (0o3345, 0o3613))      # no stock code: state mask of 10 bits, two bytes skipped, served by PLAN_LDS2
MASK_3_4 = (1, 1, 0, 1, 1, 0)       # DVB-S rate 3/4 on a rate 1/2 mother code: X 1 0 1 / Y 1 1 0, step-major

# name: code (an index into COMMON_CODES or a Code), decode type, Eb/N0 of the mother code's symbols, mask, rotations, windows, extra
# steps, the truth, seed.  K = 7: W = 64 and the default extension 48; otherwise the smallest window the default extension 8 (K-1)
# allows.  `extra` makes T non-uniform.  Behind the int8 cases and the two K: error rate of the winner / of the best hypothesis not
# equivalent to the truth, on the reference
CASES = {
    "voyager":      dict(code=VOYAGER, decode_type="SOFT16", ebn0=4.0, mask=None, rotations="qpsk", windows=4, extra=0, truth=(1, SWAP | NEG_EVEN), seed=1),
    "voyager_3_4":  dict(code=VOYAGER, decode_type="SOFT16", ebn0=5.5, mask=MASK_3_4, rotations="bpsk", windows=4, extra=0, truth=(3, NEG_EVEN | NEG_ODD), seed=2),
    "lte":          dict(code=LTE, decode_type="SOFT16", ebn0=4.0, mask=None, rotations="bpsk", windows=4, extra=0, truth=(2, 0), seed=3),
    "is95":         dict(code=IS95, decode_type="SOFT16", ebn0=4.0, mask=None, rotations="qpsk", windows=4, extra=0, truth=(1, NEG_EVEN | NEG_ODD), seed=4),
    "cassini":      dict(code=CASSINI, decode_type="SOFT16", ebn0=8.0, mask=None, rotations="none", windows=4, extra=0, truth=(4, 0), seed=5),
    "voyager_long": dict(code=VOYAGER, decode_type="SOFT16", ebn0=4.0, mask=None, rotations="bpsk", windows=4, extra=21, truth=(1, 0), seed=6),
    "voy_soft8":    dict(code=VOYAGER, decode_type="SOFT8", ebn0=5.0, mask=None, rotations="qpsk", windows=4, extra=0, truth=(1, SWAP | NEG_EVEN), seed=11),   # 0.017 / 0.146
    # HARD8: the channel's noise symbols land on the midpoint 0, so `compared` differs between the hypotheses (378 .. 380)
    "voy_hard8":    dict(code=VOYAGER, decode_type="HARD8", ebn0=6.0, mask=None, rotations="qpsk", windows=4, extra=0, truth=(0, SWAP | NEG_ODD), seed=12),    # 0.003 / 0.076
    "lte_soft8":    dict(code=LTE, decode_type="SOFT8", ebn0=5.0, mask=None, rotations="bpsk", windows=4, extra=5, truth=(1, 0), seed=13),                     # 0.036 / 0.195
    "dab_hard8":    dict(code=DAB, decode_type="HARD8", ebn0=6.0, mask=None, rotations="bpsk", windows=4, extra=3, truth=(3, 0), seed=14),                     # 0.018 / 0.154
    "voy34_hard8":  dict(code=VOYAGER, decode_type="HARD8", ebn0=7.5, mask=MASK_3_4, rotations="qpsk", windows=4, extra=7, truth=(2, SWAP | NEG_EVEN), seed=15),  # 0.000 / 0.017
    "k5":           dict(code=K5, decode_type="SOFT16", ebn0=5.0, mask=None, rotations="qpsk", windows=4, extra=0, truth=(1, SWAP | NEG_ODD), seed=16),       # 0.025 / 0.138
    "k11_lds2":     dict(code=K11, decode_type="SOFT16", ebn0=4.0, mask=None, rotations="bpsk", windows=4, extra=0, truth=(1, NEG_EVEN | NEG_ODD), seed=17),   # 0.056 / 0.176
}
CPU_CASES = ["voyager", "voyager_3_4", "lte", "is95", "cassini", "voy_soft8", "voy_hard8", "lte_soft8", "dab_hard8", "voy34_hard8", "k5",
             "k11_lds2"]


ALL_FLAGS_64 = [(offset, flags) for offset in range(8) for flags in range(8)]
# the hypothesis counts of tests/test_gpu_sync_search.py on the `voyager` case: every lane of the start-state and ranking kernels, the
# same with the winner in another lane, and one lane
CASES["voyager_64"] = dict(CASES["voyager"], hypotheses=ALL_FLAGS_64)
CASES["voyager_64_reversed"] = dict(CASES["voyager"], hypotheses=ALL_FLAGS_64[::-1])
CASES["voyager_1"] = dict(CASES["voyager"], hypotheses=[CASES["voyager"]["truth"]])

# extensions and windows (K = 7, skip = 8): head != tail, both from {K-1, K, 2K+1, 8(K-1)}; W no multiple of head; T = head + windows W +
# rem + tail with rem = 1 or W - 1 steps over the window grid.  head, tail, W, windows, rem
_SHAPES = [(6, 15, 20, 3, 1), (7, 48, 50, 2, 49), (15, 6, 25, 3, 1), (48, 7, 72, 2, 71)]
# the count's first symbol sits (head + skip) R sizeof(soft_t) bytes into a row: the residue of that offset decides how enc_load reads
#                 base case     bytes per step   head 6        head 7        head 15       head 48
_SHAPE_BASES = [("voyager", 4, ("8 mod 16", "4 mod 8", "4 mod 8", "0 mod 16")),        # 56, 60, 92, 224: int16 R = 2 allows no other
                ("voy_soft8", 2, ("4 mod 8", "2 mod 4", "2 mod 4", "0 mod 16")),       # 28, 30, 46, 112
                ("lte_soft8", 3, ("2 mod 4", "odd", "odd", "8 mod 16"))]               # 42, 45, 69, 168
SHAPE_CASES = []                                                                        # (name, residue of the byte offset)
for _base, _step_bytes, _residues in _SHAPE_BASES:
    for (_head, _tail, _W, _windows, _rem), _residue in zip(_SHAPES, _residues):
        _name = f"{_base}_head{_head}"
        CASES[_name] = dict(CASES[_base], ebn0=SHAPE_EBN0, shape=(_W, _head, _tail, _head + _windows * _W + _rem + _tail))
        SHAPE_CASES.append((_name, _residue))


def residue_class(offset_bytes):
    """the widest access enc_load can make at a byte offset from a 16-byte aligned base, as SHAPE_CASES names it"""
    return "0 mod 16" if offset_bytes % 16 == 0 else "8 mod 16" if offset_bytes % 8 == 0 else "4 mod 8" if offset_bytes % 4 == 0 else \
        "2 mod 4" if offset_bytes % 2 == 0 else "odd"


@functools.lru_cache(maxsize=None)
def make_case(name):
    """the received buffer of a case and everything a search of it takes: a random stream through the AWGN quantiser, punctured,
    sent through impair(truth)"""
    spec = CASES[name]
    code = spec["code"] if isinstance(spec["code"], Code) else COMMON_CODES[spec["code"]]
    pc = get_decoding_config(spec["decode_type"], code.R)
    high, low = pc.soft_decision_high, pc.soft_decision_low
    head = tail = ext = sr.default_extension(code.K)
    W = 64 if code.K == 7 else ext
    T = ext + spec["windows"] * W + ext + spec["extra"]
    if "shape" in spec:
        W, head, tail, T = spec["shape"]
    mask = None if spec["mask"] is None else np.asarray(spec["mask"], dtype=np.uint8)
    period_steps = 1 if mask is None else mask.size // code.R
    kept = code.R if mask is None else int(mask.sum())
    hypotheses = list(spec["hypotheses"]) if "hypotheses" in spec else enumerate_hypotheses(kept, spec["rotations"])
    # the stream goes on behind T so that the later offsets read symbols, not noise: two more periods and a step, and the periods
    # that offsets beyond one period reach into
    steps = T + (2 + max(o for o, _ in hypotheses) // kept) * period_steps + 1
    bits, sym = sr.make_stream(code, pc, steps, spec["ebn0"], spec["seed"])
    flat = sym[:steps].reshape(-1)
    sent = flat if mask is None else flat[np.resize(mask.astype(bool), flat.size)]
    rng = np.random.default_rng(1000 + spec["seed"])
    received = impair(sent, *spec["truth"], high, low, rng)
    assert received.size >= needed_received(hypotheses, T, code.R, mask)
    return dict(name=name, code=code, decode_type=spec["decode_type"], pc=pc, mask=mask, hypotheses=hypotheses, T=T, W=W, head=head,
                tail=tail, received=received, truth=spec["truth"], true_index=hypotheses.index(spec["truth"]), tx_bits=bits,
                sent_stream=sym[:T])


_references = {}


def case_reference(oracle, name):
    """search_reference of a case, computed once per process and shared by the tests: (errors, compared, best, decoded bits)"""
    if name not in _references:
        c = make_case(name)
        _references[name] = search_reference(oracle, c["code"], c["decode_type"], c["received"], c["hypotheses"], c["T"], c["W"],
                                             c["head"], c["tail"], c["mask"])
    return _references[name]
