"""vit_hip_sync_build and vit_hip_sync_search on the device against tests/sync_reference.py: every symbol of the built streams
(widths, rates, masks, offsets, flag sets, the clamp, a pitch behind the steps, one and 64 hypotheses, a map too long for LDS), the
counts and the winner of the search EQUAL to the reference's for the cases of tests/test_sync_cpu.py on the register plan, PLAN_LDS2
and the forced PLAN_LDS, a longer last window, the call captured into a graph and replayed on a second buffer, every argument
rejection with the outputs untouched, and the winning hypothesis fed to decode_stream.  The int8 widths (the channel's noise on the
midpoint under HARD8), a state of half a byte and one of 10 bits, 64 hypotheses, one, and extensions and windows that put the count's
first symbol at every alignment enc_load tells apart run the same comparison."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, _lib
from viterbidecodercpp_amd.codes import Code
from viterbidecodercpp_amd.sync import NEG_EVEN, NEG_ODD, SWAP
from tests import sync_reference as ref
from tests.helpers import DECODE_TYPES, make_table_config, sync_search_raw

pytestmark = pytest.mark.gpu

CODE_OF_RATE = {2: ref.VOYAGER, 3: ref.LTE, 4: 4}


@functools.lru_cache(maxsize=None)
def decoder(code_id, decode_type, plan=_lib.PLAN_AUTO):
    code = code_id if isinstance(code_id, Code) else COMMON_CODES[code_id]
    pc, table, config = make_table_config(code, decode_type)
    return code, pc, BatchDecoder(table, config, plan=plan)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_received(pc, n, rng):
    """symbols over the whole range of the type, its minimum (which negation clamps) among them"""
    info = np.iinfo(pc.soft_dtype)
    rec = rng.integers(info.min, info.max + 1, size=n).astype(pc.soft_dtype)
    rec[rng.integers(0, n, size=max(n // 16, 4))] = info.min
    return rec


def check_build(dec, pc, R, received, hyps, T, mask, pitch):
    import torch
    high, low = pc.soft_decision_high, pc.soft_decision_low
    d_rec = cuda(received)
    if pitch is None:
        got = dec.sync_build(d_rec, hyps, T, mask=mask).cpu().numpy()
        assert got.shape == (len(hyps), T, R)
    else:
        poison = 0x55 if pc.soft_dtype == np.int8 else 0x5555
        out = torch.full((len(hyps), pitch, R), poison, dtype=d_rec.dtype, device="cuda")
        assert dec.sync_build(d_rec, hyps, T, mask=mask, pitch=pitch, out=out) is out
        got = out.cpu().numpy()
        assert (got[:, T:] == poison).all(), "steps behind T were written"
    for i, (offset, flags) in enumerate(hyps):
        want = ref.build_stream(received, offset, flags, T, R, high, low, mask)
        bad = np.argwhere(got[i, :T] != want)
        assert bad.size == 0, f"hypothesis {i} {(offset, flags)}: first of {len(bad)} differing symbols at (step, i) = {bad[0]}"


@pytest.mark.parametrize("decode_type", DECODE_TYPES)
@pytest.mark.parametrize("R", [2, 3, 4])
def test_sync_build(R, decode_type):
    """T R is no multiple of the period, the period (5 steps) no multiple of the 16-byte store, more than one workgroup per
    hypothesis, offsets 0 and kept - 1 under all 8 flag sets; rows at 16-byte multiples and not; steps behind T untouched"""
    code, pc, dec = decoder(CODE_OF_RATE[R], decode_type)
    assert code.R == R
    rng = np.random.default_rng(10 * R + len(decode_type))
    T = 2503
    for mask in (None, rng.integers(0, 2, size=5 * R).astype(np.uint8) | np.eye(1, 5 * R, 2, dtype=np.uint8)[0]):
        kept = R if mask is None else int(mask.sum())
        hyps = [(o, f) for o in sorted({0, kept - 1}) for f in range(8)]
        received = random_received(pc, ref.needed_received(hyps, T, R, mask) + 3, rng)
        check_build(dec, pc, R, received, hyps, T, mask, None)              # packed rows: T R sizeof(soft_t) is odd or 2 mod 4
        check_build(dec, pc, R, received, hyps, T, mask, T + 1)
        check_build(dec, pc, R, received, hyps, T, mask, 2512)              # rows 16 bytes aligned
        check_build(dec, pc, R, received, hyps[5:6], 37, mask, None)        # one hypothesis, three chunks


def test_sync_build_64_hypotheses_and_a_long_map():
    code, pc, dec = decoder(ref.VOYAGER, "SOFT16")
    rng = np.random.default_rng(64)
    T = 300
    mask = rng.integers(0, 2, size=8).astype(np.uint8) | np.uint8([1, 0, 0, 0, 0, 0, 0, 1])
    hyps = [(o, f) for o in range(8) for f in range(8)]
    received = random_received(pc, ref.needed_received(hyps, T, 2, mask) + 1, rng)
    check_build(dec, pc, 2, received, hyps, T, mask, 304)
    # 1030 map entries: read from global memory, not staged
    long_mask = rng.integers(0, 2, size=1030).astype(np.uint8)
    long_mask[0] = 1
    T = 1300
    hyps = [(0, 0), (3, SWAP | NEG_ODD), (int(long_mask.sum()) - 1, NEG_EVEN)]
    received = random_received(pc, ref.needed_received(hyps, T, 2, long_mask) + 1, rng)
    check_build(dec, pc, 2, received, hyps, T, long_mask, None)


def run_search(dec, c, received=None, **kw):
    err, cmp, best = dec.sync_search(cuda(c["received"] if received is None else received), c["hypotheses"], c["T"], mask=c["mask"],
                                     window=c["W"], head=c["head"], tail=c["tail"], **kw)
    assert best.numel() == 1 and best.is_cuda
    return err.cpu().numpy().astype(np.int64), cmp.cpu().numpy().astype(np.int64), int(best.item())


SEARCHES = [(name, _lib.PLAN_LDS2 if name == "k11_lds2" else _lib.PLAN_AUTO) for name in ref.CPU_CASES + ["voyager_long"]] + [
    ("voyager", _lib.PLAN_LDS), ("voyager_3_4", _lib.PLAN_LDS), ("voy_hard8", _lib.PLAN_LDS), ("lte_soft8", _lib.PLAN_LDS)]


@pytest.mark.parametrize("name,plan", SEARCHES)
def test_sync_search_equals_the_reference(oracle, name, plan):
    c = ref.make_case(name)
    want_err, want_cmp, want_best, _ = ref.case_reference(oracle, name)
    code, pc, dec = decoder(c["code"], c["decode_type"], plan)
    assert dec.plan == {("cassini", _lib.PLAN_AUTO): _lib.PLAN_LDS2}.get((name, plan), plan or _lib.PLAN_REG)
    err, cmp, best = run_search(dec, c)
    assert err.tolist() == want_err.tolist() and cmp.tolist() == want_cmp.tolist(), (err, want_err, cmp, want_cmp)
    assert best == want_best
    if name == "voy_hard8":
        assert len(set(cmp.tolist())) > 1, "the hypotheses were to compare different numbers of symbols"
    need = dec.sync_search_workspace_bytes(len(c["hypotheses"]), c["T"], c["W"], c["head"], c["tail"])
    assert need > 0 and need % 256 == 0


@pytest.mark.parametrize("name", ["voyager_64", "voyager_64_reversed", "voyager_1"])
def test_sync_search_hypothesis_counts(oracle, name):
    """64 hypotheses (offsets 0 .. 7 under all 8 flag sets: every lane of the start-state and ranking kernels, 64 streams in the
    decode, the largest workspace), the same list reversed (the winner in another lane) and the truth alone.  The outputs are three
    slices of one poisoned buffer: what lies between and behind them is as it was"""
    import torch
    c = ref.make_case(name)
    n = len(c["hypotheses"])
    want_err, want_cmp, want_best, _ = ref.case_reference(oracle, name)
    code, pc, dec = decoder(c["code"], c["decode_type"])
    POISON = -7
    buf = torch.full((256,), POISON, dtype=torch.int32, device="cuda")
    e0, c0, b0 = 3, 3 + n + 13, 3 + n + 13 + n + 6                    # 3 in front, 13 and 6 between, the rest behind
    need = dec.sync_search_workspace_bytes(n, c["T"], c["W"], c["head"], c["tail"])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert sync_search_raw(dec, c, ws.data_ptr(), need, buf[e0:e0 + n], buf[c0:c0 + n], buf[b0:b0 + 1]) == _lib.OK
    host = buf.cpu().numpy().astype(np.int64)
    assert host[e0:e0 + n].tolist() == want_err.tolist() and host[c0:c0 + n].tolist() == want_cmp.tolist()
    best = int(host[b0])
    assert best == want_best and ref.aligned(c, c["hypotheses"][best])
    if n == 1:
        assert best == 0
    written = np.zeros(host.size, dtype=bool)
    written[e0:e0 + n] = written[c0:c0 + n] = written[b0] = True
    assert written[:b0 + 1].sum() == 2 * n + 1 and (host[~written] == POISON).all(), np.flatnonzero((host != POISON) & ~written)
    if name == "voyager_64_reversed":
        assert best != ref.case_reference(oracle, "voyager_64")[2]


@pytest.mark.parametrize("name,residue", ref.SHAPE_CASES)
def test_sync_search_extensions_and_windows(oracle, name, residue):
    """head != tail from {K-1, K, 2K+1, 8(K-1)}, W no multiple of head, a last window 1 or W - 1 steps longer: the count's first
    symbol sits `residue` bytes into a row (ref.SHAPE_CASES lists them; tests/test_sync_cpu.py checks the list), rows at pitches that
    are no multiple of 16 bytes.  Short extensions decode poorly -- the reference's decode is as poor, and the counts are equal"""
    c = ref.make_case(name)
    want_err, want_cmp, want_best, _ = ref.case_reference(oracle, name)
    code, pc, dec = decoder(c["code"], c["decode_type"])
    assert dec.plan == _lib.PLAN_REG
    err, cmp, best = run_search(dec, c)
    assert err.tolist() == want_err.tolist() and cmp.tolist() == want_cmp.tolist(), (residue, err, want_err, cmp, want_cmp)
    assert best == want_best and ref.equivalent(code, c["hypotheses"][best], c["truth"])


def test_sync_search_captured_into_a_graph(oracle):
    """one capture on one stream, replayed on a second received buffer (another stream through another channel: another winner)"""
    import torch
    c = ref.make_case("voyager")
    code, pc, dec = decoder(ref.VOYAGER, "SOFT16")
    first = c["received"]
    second = ref.make_case("voyager_long")["received"][:first.size].copy()
    assert second.size == first.size
    wants = [ref.case_reference(oracle, "voyager")[:3],
             ref.search_reference(oracle, code, "SOFT16", second, c["hypotheses"], c["T"], c["W"], c["head"], c["tail"])[:3]]
    assert wants[1][2] != wants[0][2]
    d_rec = cuda(first)
    args = dict(mask=None, window=c["W"], head=c["head"], tail=c["tail"])
    ws = torch.empty(dec.sync_search_workspace_bytes(len(c["hypotheses"]), c["T"], c["W"], c["head"], c["tail"]), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.sync_search(d_rec, c["hypotheses"], c["T"], workspace=ws, **args)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        err, cmp, best = dec.sync_search(d_rec, c["hypotheses"], c["T"], workspace=ws, **args)
    for rec, want in zip((first, second), wants):
        d_rec.copy_(cuda(rec))
        err.fill_(-1), cmp.fill_(-1), best.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert err.cpu().numpy().tolist() == want[0].tolist() and cmp.cpu().numpy().tolist() == want[1].tolist()
        assert int(best.item()) == want[2]


def test_ranking_on_the_device_with_nothing_compared():
    """SOFT16 symbols all at the midpoint: every hypothesis compares nothing, nobody beats anybody, index 0 wins"""
    code, pc, dec = decoder(ref.VOYAGER, "SOFT16")
    c = ref.make_case("voyager")
    err, cmp, best = run_search(dec, c, received=np.zeros_like(c["received"]))
    assert not err.any() and not cmp.any() and best == 0


def test_rejections_launch_nothing():
    """every rejected call returns its code and leaves errors, compared, best and the workspace as they were"""
    import torch
    c = ref.make_case("voyager")
    code, pc, dec = decoder(ref.VOYAGER, "SOFT16")
    lib, h = _lib.load(), dec._handle._h
    T, W, head, tail = c["T"], c["W"], c["head"], c["tail"]
    hyps = c["hypotheses"]
    n = len(hyps)
    d_rec = cuda(c["received"])
    need = lib.vit_hip_sync_search_workspace_bytes(h, n, T, W, head, tail)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((3, 64), -7, dtype=torch.int32, device="cuda")
    d_map = cuda(ref.source_map(ref.MASK_3_4)[0])
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def search(n_received=d_rec.numel(), source=None, period=0, kept=0, hyps=hyps, n_hyp=None, T=T, W=W, head=head, tail=tail, ws_bytes=need):
        arr = (_lib.VitHipSyncHypothesis * max(len(hyps), 1))(*hyps)
        return lib.vit_hip_sync_search(h, ptr(d_rec), n_received, source, period, kept, arr, len(hyps) if n_hyp is None else n_hyp, T, W, head,
                                       tail, ptr(ws), ws_bytes, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream)

    INV, WS = _lib.ERR_INVALID_ARG, _lib.ERR_WORKSPACE
    exact = ref.needed_received(hyps, T, 2)
    assert exact <= d_rec.numel()
    many = [(0, 0)] * 65
    cases = {
        "read past n_received": (search(n_received=exact - 1), INV),
        "no hypothesis": (search(n_hyp=0), INV),
        "65 hypotheses": (search(hyps=many), INV),
        "unknown flag bits": (search(hyps=[(0, 8)]), INV),
        "n_out <= skip": (search(T=head + tail + 8), INV),
        "short workspace": (search(ws_bytes=need - 1), WS),
        "period % R": (search(source=ptr(d_map), period=5, kept=4), INV),
        "kept > period": (search(source=ptr(d_map), period=6, kept=7), INV),
        "head < K-1": (search(head=5), INV),
    }
    torch.cuda.synchronize()
    for what, (rc, want) in cases.items():
        assert rc == want, (what, rc)
    assert (out == -7).all().item() and (ws == 0xA5).all().item()
    cases.clear()
    assert search(n_received=exact) == _lib.OK                   # the bound is tight, and a passing call does write
    torch.cuda.synchronize()
    assert (out[:2, :n] >= 0).all().item() and 0 <= int(out[2, 0]) < n
    out.fill_(-7), ws.fill_(0xA5)
    # the build alone: the same checks, and a pitch below T
    sym = torch.full((n, T, 2), 0x5555, dtype=torch.int16, device="cuda")
    arr = (_lib.VitHipSyncHypothesis * n)(*hyps)
    build = lambda n_received=d_rec.numel(), n_hyp=n, pitch=T, a=arr: lib.vit_hip_sync_build(h, ptr(d_rec), n_received, None, 0, 0, a, n_hyp, T, pitch, ptr(sym), stream)
    cases["build: read past n_received"] = (build(n_received=exact - 1), INV)
    cases["build: no hypothesis"] = (build(n_hyp=0), INV)
    cases["build: 65 hypotheses"] = (lib.vit_hip_sync_build(h, ptr(d_rec), d_rec.numel(), None, 0, 0, (_lib.VitHipSyncHypothesis * 65)(*many), 65, T, T, ptr(sym), stream), INV)
    cases["build: unknown flag bits"] = (build(n_hyp=1, a=(_lib.VitHipSyncHypothesis * 1)((0, 16))), INV)
    cases["build: pitch < T"] = (build(pitch=T - 1), INV)
    cases["build: period % R"] = (lib.vit_hip_sync_build(h, ptr(d_rec), d_rec.numel(), ptr(d_map), 3, 2, arr, n, T, T, ptr(sym), stream), INV)
    torch.cuda.synchronize()
    for what, (rc, want) in cases.items():
        assert rc == want, (what, rc)
    assert (out == -7).all().item() and (ws == 0xA5).all().item() and (sym == 0x5555).all().item()
    assert lib.vit_hip_sync_search_workspace_bytes(h, n, head + tail + 8, W, head, tail) == 0
    assert lib.vit_hip_sync_search_workspace_bytes(h, 65, T, W, head, tail) == 0
    assert lib.vit_hip_sync_search_workspace_bytes(h, 0, T, W, head, tail) == 0
    with pytest.raises(_lib.VitHipError):
        dec.sync_search(d_rec[:exact - 1].contiguous(), hyps, T, window=W, head=head, tail=tail)
    with pytest.raises(ValueError):
        dec.sync_search(d_rec, hyps, head + tail + 8, window=W, head=head, tail=tail)


@pytest.mark.parametrize("name", ["voyager", "lte", "voyager_3_4"])
def test_the_winning_hypothesis_decodes_to_the_data(name):
    """the winner, built alone at pitch = steps, is the stream decode_stream reads: its bits are the transmitted data (inverted when
    the channel inverted a transparent code and the tie went to the upright hypothesis)"""
    c = ref.make_case(name)
    code, pc, dec = decoder(c["code"], c["decode_type"])
    err, cmp, best = run_search(dec, c)
    winner = c["hypotheses"][best]
    assert ref.equivalent(code, winner, c["truth"])
    stream = dec.sync_build(cuda(c["received"]), [winner], c["T"], mask=c["mask"])
    out, n_bits = dec.decode_stream(stream[0], begin=False, end=False, window=c["W"], head=c["head"], tail=c["tail"])
    bits = np.unpackbits(out.cpu().numpy())[:n_bits]
    tx = c["tx_bits"][c["head"]:c["T"] - c["tail"]]
    inverted = winner != c["truth"]
    assert inverted == (name == "voyager_3_4")
    assert np.array_equal(bits ^ int(inverted), tx)
