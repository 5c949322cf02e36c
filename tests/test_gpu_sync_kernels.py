"""The two small kernels of node synchronisation on their own (csrc/kernels_sync.hpp: sync_pick_kernel, sync_state_kernel), on inputs
a real search never produces.  tests/cpp/sync_kernels_probe.hip includes the library's header and calls its launchers
(vit::sync_launch_pick, vit::sync_launch_state) once per set; nothing of the kernels is copied.

The ranking against sync_reference.rank: the hand-written sets of sync_reference.RANK_SETS (tests/test_sync_cpu.py pins their winners:
equal rates with other denominators, products beyond 2^32 whose low halves order the other way, nothing compared beside live
hypotheses, the winner in lane 62 and 63, one hypothesis) and 2000 random ones, half of them small integers where ties for first place
are common.  The start states against the one-line rule of sync_reference.search_reference (bit j = emitted bit skip - 1 - j) for K =
3 .. 16, at strides that are no multiple of 4 and with 1, 37 and 64 hypotheses.  All integers: equality."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import sync_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SLOTS = ref.MAX_HYPOTHESES
POISON = 0xDEADBEEF
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    path = os.path.join(HERE, "cpp", "libsync_kernels_probe.so")
    assert os.path.exists(path), "tests/cpp/libsync_kernels_probe.so is missing: make -C tests/cpp"
    lib = C.CDLL(path)
    lib.sync_probe_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, U32P, C.c_uint32, C.c_void_p]
    lib.sync_probe_state.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, U64P, U32P, U32P, U32P, C.c_uint32, C.c_void_p]
    return lib


def to_device(a):
    """uint32 / uint8 host array -> CUDA tensor of the same bits"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def pick_on_device(probe, sets):
    """sets: [(errors, compared)] or None for a set that is not launched -> best [len(sets)] uint32, POISON where nothing ran"""
    import torch
    n_sets = len(sets)
    # the slots behind n_hyp hold 0 errors of 1 compared: a kernel that ranked them would name one of them wherever a live
    # hypothesis has an error
    errors = np.zeros((n_sets, SLOTS), dtype=np.uint32)
    compared = np.ones((n_sets, SLOTS), dtype=np.uint32)
    n_hyp = np.zeros(n_sets, dtype=np.uint32)
    for s, item in enumerate(sets):
        if item is None:
            continue
        e, c = item
        n_hyp[s] = len(e)
        errors[s, :len(e)] = e
        compared[s, :len(c)] = c
    d_err, d_cmp = to_device(errors), to_device(compared)
    d_best = to_device(np.full(n_sets, POISON, dtype=np.uint32))
    rc = probe.sync_probe_pick(d_err.data_ptr(), d_cmp.data_ptr(), d_best.data_ptr(), n_hyp.ctypes.data_as(U32P), n_sets,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(to_host_u32(d_err), errors) and np.array_equal(to_host_u32(d_cmp), compared), "the ranking wrote to its inputs"
    return to_host_u32(d_best)


def test_ranking_of_the_hand_written_sets(probe):
    sets = [(e, c) for _, e, c, _ in ref.RANK_SETS]
    # every second launch is left out: its entry of `best` keeps the poison
    interleaved = [x for item in sets for x in (item, None)]
    best = pick_on_device(probe, interleaved)
    assert (best[1::2] == POISON).all()
    for (name, e, c, winner), got in zip(ref.RANK_SETS, best[0::2]):
        assert winner == ref.rank(e, c)
        assert int(got) == winner, (name, int(got), winner)


def test_ranking_of_random_sets(probe):
    """ref.random_rank_sets: tests/test_sync_cpu.py asserts what the seed gives (ties for first place in most small-integer sets,
    n = 1 and n = 64, winners off index 0); here again the tie condition, beside the comparison it is for"""
    sets = ref.random_rank_sets()
    want = [ref.rank([int(x) for x in e], [int(x) for x in c]) for e, c in sets]
    small = sets[0::2]
    ties = sum(1 for e, c in small if ref.tied_for_first(e, c) >= 2)
    assert 3 * ties >= len(small), f"only {ties} of {len(small)} small-integer sets tie for first place"
    # the last 40 sets are not launched
    launched = len(sets) - 40
    best = pick_on_device(probe, sets[:launched] + [None] * 40)
    assert (best[launched:] == POISON).all()
    wrong = [(s, int(best[s]), want[s]) for s in range(launched) if int(best[s]) != want[s]]
    assert not wrong, f"{len(wrong)} of {launched} sets, first (set, device, reference) = {wrong[0]}: errors {sets[wrong[0][0]][0]}, compared {sets[wrong[0][0]][1]}"


def state_rule(row_bytes, K):
    """search_reference's rule on the first skip bits of one hypothesis's decoded bytes"""
    skip = ref.skip_bits(K)
    bits = np.unpackbits(np.asarray(row_bytes[:skip // 8], dtype=np.uint8))
    return sum(int(bits[skip - 1 - j]) << j for j in range(K - 1))


STATE_SET_BYTES = SLOTS * 48


def state_sets():
    """(K, skip_bytes, byte_stride, n_hyp, fill) for K = 3 .. 16, the strides {skip_bytes, 17, 48}, 1, 37 and 64 hypotheses, random
    bytes and all-0xFF bytes"""
    out = []
    for K in range(3, 17):
        skip_bytes = (K - 1 + 7) // 8
        for stride in (skip_bytes, 17, 48):
            for n_hyp in (1, 37, 64):
                for fill in ("random", "ones"):
                    out.append((K, skip_bytes, stride, n_hyp, fill))
    return out


def test_start_states(probe):
    import torch
    sets = state_sets()
    n_sets = len(sets)
    assert {s[0] for s in sets} == set(range(3, 17)) and {s[1] for s in sets} == {1, 2}
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, size=(n_sets, STATE_SET_BYTES), dtype=np.uint8)
    for s, (K, skip_bytes, stride, n_hyp, fill) in enumerate(sets):
        assert (n_hyp - 1) * stride + skip_bytes <= STATE_SET_BYTES                  # what the kernel reads lies inside its set
        if fill == "ones":
            data[s] = 0xFF
    # one more set than is launched: its outputs keep the poison
    state = np.full((n_sets + 1, SLOTS), POISON, dtype=np.uint32)
    d_bytes, d_state, d_err, d_cmp = to_device(data), to_device(state), to_device(state), to_device(state)
    strides = np.array([s[2] for s in sets], dtype=np.uint64)
    n_hyps = np.array([s[3] for s in sets], dtype=np.uint32)
    skips = np.array([s[1] for s in sets], dtype=np.uint32)
    Ks = np.array([s[0] for s in sets], dtype=np.uint32)
    rc = probe.sync_probe_state(d_bytes.data_ptr(), STATE_SET_BYTES, d_state.data_ptr(), d_err.data_ptr(), d_cmp.data_ptr(),
                                strides.ctypes.data_as(U64P), n_hyps.ctypes.data_as(U32P), skips.ctypes.data_as(U32P),
                                Ks.ctypes.data_as(U32P), n_sets, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(d_bytes.cpu().numpy(), data)
    got, err, cmp = to_host_u32(d_state), to_host_u32(d_err), to_host_u32(d_cmp)
    for s, (K, skip_bytes, stride, n_hyp, fill) in enumerate(sets):
        want = [state_rule(data[s, h * stride:h * stride + skip_bytes], K) for h in range(n_hyp)]
        if fill == "ones":
            assert want == [(1 << (K - 1)) - 1] * n_hyp
        assert got[s, :n_hyp].tolist() == want, (sets[s], got[s, :n_hyp].tolist(), want)
        assert not err[s, :n_hyp].any() and not cmp[s, :n_hyp].any(), (sets[s], "the counters were to be zeroed")
        for what, a in (("state", got), ("errors", err), ("compared", cmp)):
            assert (a[s, n_hyp:] == POISON).all(), (sets[s], what, "written behind n_hyp")
    assert (got[n_sets] == POISON).all() and (err[n_sets] == POISON).all() and (cmp[n_sets] == POISON).all()
