"""SURVEY 8 f-1 / f-2 on the device: the frame generator (vit_hip_synth_batch), the bit-error counter and the BER sweep driver,
checked against the reference's encoder (oracle/_ref), the C restatement, and the numpy mirror of the generator."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, _lib, synth
from viterbidecodercpp_amd.codes import Code
from viterbidecodercpp_amd.tools import run_snr_ber
from tests.helpers import make_table_config, oracle_cfg

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
# rates 1, 5, 7 and 8 of with_rate and the two ends of K, which no stock code has: any polynomials with the top and the bottom bit set
EXTRA_CODES = {
    "R1": Code("K5R1", 5, 1, (0o27,)),
    "R5": Code("K5R5", 5, 5, (0o25, 0o27, 0o33, 0o35, 0o37)),
    "R7": Code("K7R7", 7, 7, (0o133, 0o145, 0o175, 0o117, 0o127, 0o155, 0o171)),
    "R8": Code("K4R8", 4, 8, (0o11, 0o13, 0o15, 0o17, 0o13, 0o11, 0o17, 0o15)),
    "K2": Code("K2R2", 2, 2, (0o3, 0o3)),
    "K16": Code("K16R2", 16, 2, (46749, 58851)),
}


@functools.lru_cache(maxsize=None)
def extra_decoder(name, decode_type):
    """(code, pc, decoder) of a code outside the stock table, on the plan that needs no kernels made for its polynomials"""
    code = EXTRA_CODES[name]
    pc, table, config = make_table_config(code, decode_type)
    return code, pc, BatchDecoder(table, config, plan=_lib.PLAN_LDS2 if code.K >= 10 else _lib.PLAN_LDS)


@pytest.mark.parametrize("code_id", range(8))
@pytest.mark.parametrize("decode_type", ["SOFT16", "HARD8"])
def test_noise_free_frames_equal_the_reference_encoder(oracle, code_id, decode_type):
    code = COMMON_CODES[code_id]
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    F, L = 7, 8 * 37
    tx, sym = dec.synth(F, L, None, seed=11, first_frame=3)
    tx, sym = tx.cpu().numpy(), sym.cpu().numpy()
    want_tx, want_sym = synth.make_frames_philox_numpy(code, pc, F, L, None, seed=11, first_frame=3)
    assert np.array_equal(tx, want_tx) and np.array_equal(sym, want_sym)
    # ... and the symbols are what the reference's encoders make of those bytes (encode_data, test_helpers.h:17-64)
    from oracle import pyoracle
    ref = pyoracle.RefLib() if pyoracle.RefLib.available() else None
    for f in range(F):
        bits = oracle.encode(code.K, code.R, code.G, tx[f]).reshape(-1, code.R)
        assert np.array_equal(sym[f], np.where(bits != 0, pc.soft_decision_high, pc.soft_decision_low))
        if ref is not None:
            for which in (0, 1):        # ConvolutionalEncoder_ShiftRegister, ConvolutionalEncoder_Lookup
                assert np.array_equal(ref.encode(code_id, tx[f], which).reshape(-1, code.R), bits)


def test_batch_does_not_depend_on_how_it_is_split():
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    import torch
    tx, sym = dec.synth(16, 1024, 2.0, seed=5)
    tx_a, sym_a = dec.synth(9, 1024, 2.0, seed=5, first_frame=0)
    tx_b, sym_b = dec.synth(7, 1024, 2.0, seed=5, first_frame=9)
    assert torch.equal(tx, torch.cat([tx_a, tx_b])) and torch.equal(sym, torch.cat([sym_a, sym_b]))
    tx2, sym2 = dec.synth(16, 1024, 2.0, seed=6)
    assert not torch.equal(tx, tx2)


@pytest.mark.parametrize("code_id,decode_type,ebn0", [(2, "SOFT16", 3.0), (2, "HARD8", 5.0), (3, "SOFT8", 2.0), (7, "SOFT16", -4.0),
                                                      (6, "SOFT16", 0.0)])
def test_noisy_frames_follow_the_reference_channel_and_quantiser(code_id, decode_type, ebn0):
    """run_snr_ber.cpp:311-359.  Against the numpy mirror: identical except where the device's float32 log/sincos differ in
    the last place AND the value sits on a rounding boundary; and the first two moments of the noise are the channel's."""
    code = COMMON_CODES[code_id]
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    F, L = 64, 2048
    tx, sym = dec.synth(F, L, ebn0, seed=2024)
    tx, sym = tx.cpu().numpy(), sym.cpu().numpy().astype(np.int32)
    want_tx, want_sym = synth.make_frames_philox_numpy(code, pc, F, L, ebn0, seed=2024)
    assert np.array_equal(tx, want_tx)
    diff = np.abs(sym - want_sym.astype(np.int32))
    assert diff.max() <= 1 and (diff != 0).mean() < 1e-3, (diff.max(), (diff != 0).mean())
    # unclamped SOFT16 values: (sym - mean)/scale = +-1 + sigma z.  Estimate sigma from the symbols that are not clamped.
    if decode_type == "SOFT16":
        var = synth.noise_variance(ebn0, code.R)
        scale = 127.0 / np.sqrt(1.0 + var)
        coded = synth.encode_bits_numpy(code.K, code.R, code.G, tx)
        x = sym / scale - (2.0 * coded - 1.0)
        inside = np.abs(sym) < 127
        if inside.mean() > 0.9:      # little clipping: the sample moments are the channel's
            assert abs(x[inside].mean()) < 0.01
            assert abs(x[inside].std() / np.sqrt(var) - 1.0) < 0.03
    assert sym.max() <= pc.soft_decision_high and sym.min() >= pc.soft_decision_low


def test_bit_error_counter():
    import torch
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    rng = np.random.default_rng(3)
    # the second trip of the grid-stride loop: the grid is capped at 4096 blocks x 256 lanes x 16 bytes = 16 MiB.  The bytes are made
    # on the device, the expected count by numpy on one host copy; then one bit more in the first trip, the second trip and the tail
    n = (16 << 20) + 4099
    gen = torch.Generator(device="cuda").manual_seed(17)
    a = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    b = a ^ torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    want = int(np.unpackbits((a ^ b).cpu().numpy()).sum(dtype=np.int64))
    assert abs(want - 4 * n) < n // 100                       # random bytes: half of the bits differ
    assert int(dec.count_bit_errors(a, b).item()) == want
    for at in (0, (16 << 20) - 1, (16 << 20) + 5, (16 << 20) + 4095, n - 1):
        want += 1 if int(a[at].item()) & 0x10 == int(b[at].item()) & 0x10 else -1
        a[at] ^= 0x10
        assert int(dec.count_bit_errors(a, b).item()) == want, at
    del a, b
    # mixed alignment: one operand 16-aligned, the other not; and fewer than 16 bytes with both aligned
    base_a = torch.from_numpy(rng.integers(0, 256, 4099 + 16, dtype=np.uint8)).cuda()
    base_b = torch.from_numpy(rng.integers(0, 256, 4099 + 16, dtype=np.uint8)).cuda()
    assert base_a.data_ptr() % 16 == 0 and base_b.data_ptr() % 16 == 0
    host_a, host_b = base_a.cpu().numpy(), base_b.cpu().numpy()
    for n in (1, 15, 16, 17, 31, 4099):
        for oa, ob in ((0, 1), (1, 0)):
            want = int(np.unpackbits(host_a[oa:oa + n] ^ host_b[ob:ob + n]).sum())
            assert int(dec.count_bit_errors(base_a[oa:oa + n], base_b[ob:ob + n]).item()) == want, (n, oa, ob)
    assert int(dec.count_bit_errors(base_a[:5], base_b[:5]).item()) == int(np.unpackbits(host_a[:5] ^ host_b[:5]).sum())
    # the count word: accumulation into a non-zero count inside a poisoned int64 buffer whose neighbours stay; n = 0 and the NULL rules
    lib, h = _lib.load(), dec._handle._h
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    poison = int(np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0])
    words = torch.full((9,), poison, dtype=torch.int64, device="cuda")
    words[4] = 1 << 40
    cnt = words.data_ptr() + 4 * 8
    want = int(np.unpackbits(host_a[:4099] ^ host_b[:4099]).sum())
    assert lib.vit_hip_count_bit_errors(h, base_a.data_ptr(), base_b.data_ptr(), 4099, cnt, stream) == _lib.OK
    assert lib.vit_hip_count_bit_errors(h, base_a.data_ptr(), base_b.data_ptr(), 0, cnt, stream) == _lib.OK
    assert lib.vit_hip_count_bit_errors(h, None, None, 0, None, stream) == _lib.OK
    for args in ((None, base_b.data_ptr(), cnt), (base_a.data_ptr(), None, cnt), (base_a.data_ptr(), base_b.data_ptr(), None)):
        assert lib.vit_hip_count_bit_errors(h, args[0], args[1], 4099, args[2], stream) == _lib.ERR_INVALID_ARG, args
    assert lib.vit_hip_count_bit_errors(None, base_a.data_ptr(), base_b.data_ptr(), 4099, cnt, stream) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert words.tolist() == [poison] * 4 + [(1 << 40) + want] + [poison] * 4
    for n in (1, 15, 16, 17, 4099, 1 << 20):
        a = rng.integers(0, 256, n, dtype=np.uint8)
        b = rng.integers(0, 256, n, dtype=np.uint8)
        cnt = dec.count_bit_errors(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
        cnt = dec.count_bit_errors(torch.from_numpy(a).cuda(), torch.from_numpy(a).cuda(), cnt)     # accumulates
        assert int(cnt.item()) == int(np.unpackbits(a ^ b).sum())
    # unaligned views
    a = torch.from_numpy(rng.integers(0, 256, 1000, dtype=np.uint8)).cuda()
    b = torch.from_numpy(rng.integers(0, 256, 1000, dtype=np.uint8)).cuda()
    want = int(np.unpackbits(a[3:].cpu().numpy() ^ b[3:].cpu().numpy()).sum())
    assert int(dec.count_bit_errors(a[3:], b[3:]).item()) == want


@pytest.mark.parametrize("code_id,decode_type,points", [(2, "SOFT16", (0.0, 2.0)), (2, "HARD8", (2.0, 4.0)), (5, "SOFT16", (0.0, 1.0))])
def test_ber_point_equals_the_oracle_decoding_the_same_frames(oracle, code_id, decode_type, points):
    """tools/run_snr_ber.py: the BER the sweep reports at a point is exactly the BER of the CPU checker on the same frames."""
    code = COMMON_CODES[code_id]
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    L, frames = 512 * 8, 96
    for k, ebn0 in enumerate(points):
        seed = 40 + k
        errors, bits, batches = run_snr_ber.ber_point(dec, L, frames, ebn0, seed, max_bits=2 * frames * L, max_error_bits=1 << 40)
        assert batches == 2 and bits == 2 * frames * L
        want_errors = 0
        for b in range(batches):
            tx, sym = dec.synth(frames, L, ebn0, seed=seed, first_frame=b * frames)
            got, _, _ = oracle.decode_frames(code.K, code.R, code.G, oracle_cfg(decode_type, code.R), sym.cpu().numpy(), L, threads=8)
            want_errors += int(np.unpackbits(got ^ tx.cpu().numpy()).sum())
        assert errors == want_errors
        if ebn0 <= 2.0:
            assert errors > 0          # the points are noisy enough to mean something
    # the early-stop rule (run_snr_ber.cpp:372)
    errors, bits, batches = run_snr_ber.ber_point(dec, L, frames, points[0], 99, max_bits=10 * frames * L, max_error_bits=1)
    assert batches == 1 and errors >= 1


# ---- the generator at the rates, constraint lengths, counter words, addresses and arguments the stock codes never reach -----------------

def synth_raw(dec, F, L, seed=1, first_frame=0, ebn0=None, tx=None, sym=None):
    """vit_hip_synth_batch through the C ABI with the caller's addresses (None: NULL); synchronises and returns the call's code"""
    import torch
    rc = _lib.load().vit_hip_synth_batch(dec._handle._h, F, L, seed, first_frame, 0.0 if ebn0 is None else float(ebn0), 1 if ebn0 is None else 0,
                                         tx, sym, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name,decode_type", [("R1", "SOFT16"), ("R5", "SOFT8"), ("R7", "SOFT16"), ("R8", "HARD8"), ("K2", "SOFT16"), ("K16", "SOFT8"),
                                              (2, "SOFT8"), (6, "SOFT8")], ids=str)
def test_noise_free_frames_of_other_rates_and_lengths(oracle, name, decode_type):
    """device = mirror = the oracle's encoder for R = 1, 5, 7, 8 and K = 2, 16, and SOFT8 on two stock codes; L = 0 is the K - 1 tail
    steps alone with no info byte"""
    if isinstance(name, int):
        code = COMMON_CODES[name]
        pc, table, config = make_table_config(code, decode_type)
        dec = BatchDecoder(table, config)
    else:
        code, pc, dec = extra_decoder(name, decode_type)
    F = 5
    for L in (0, 8, 24, 296):
        tx, sym = dec.synth(F, L, None, seed=21, first_frame=6)
        tx, sym = tx.cpu().numpy(), sym.cpu().numpy()
        want_tx, want_sym = synth.make_frames_philox_numpy(code, pc, F, L, None, seed=21, first_frame=6)
        assert tx.shape == (F, L // 8) and sym.shape == (F, L + code.K - 1, code.R)
        assert np.array_equal(tx, want_tx) and np.array_equal(sym, want_sym), L
        for f in range(F):
            bits = oracle.encode(code.K, code.R, code.G, tx[f]).reshape(-1, code.R)
            assert np.array_equal(sym[f], np.where(bits != 0, pc.soft_decision_high, pc.soft_decision_low)), (L, f)
        if L == 0:
            assert (sym == pc.soft_decision_low).all()


def _close_to_the_mirror(tag, sym, want_sym):
    """the bound of test_noisy_frames_follow_the_reference_channel_and_quantiser, with the figures printed first"""
    diff = np.abs(sym.astype(np.int32) - want_sym.astype(np.int32))
    print(tag, "max difference", int(diff.max()), "share of differing symbols", float((diff != 0).mean()), "of", diff.size)
    assert diff.max() <= 1 and (diff != 0).mean() < 1e-3, (tag, diff.max(), (diff != 0).mean())


def test_frame_and_seed_reach_their_own_counter_and_key_words():
    """first_frame straddling 2^32 (the carry into the fourth counter word) and seeds with a high word (the second key word): info
    bytes equal to the mirror, noisy symbols within the project's bound of it; seeds that differ only in the high word differ"""
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    F, L = 4, 2048
    for first in ((1 << 32) - 2, (1 << 32) + 5):
        tx, sym = dec.synth(F, L, 3.0, seed=77, first_frame=first)
        want_tx, want_sym = synth.make_frames_philox_numpy(code, pc, F, L, 3.0, seed=77, first_frame=first)
        assert np.array_equal(tx.cpu().numpy(), want_tx), first
        _close_to_the_mirror(("first_frame", first), sym.cpu().numpy(), want_sym)
        free_tx, free_sym = dec.synth(F, L, None, seed=77, first_frame=first)
        assert np.array_equal(free_tx.cpu().numpy(), want_tx)
        assert np.array_equal(free_sym.cpu().numpy(), synth.make_frames_philox_numpy(code, pc, F, L, None, seed=77, first_frame=first)[1])
    # frames 2^32 - 2 .. 2^32 + 1 are four different frames, and none of them is frame 0 or 1 again
    low_tx = dec.synth(F, L, None, seed=77, first_frame=0)[0].cpu().numpy()
    high_tx = dec.synth(F, L, None, seed=77, first_frame=(1 << 32) - 2)[0].cpu().numpy()
    assert len({r.tobytes() for r in np.concatenate([low_tx, high_tx])}) == 2 * F
    got = {}
    for seed in (1, 1 << 32, (1 << 63) + 1):
        tx, sym = dec.synth(F, L, 3.0, seed=seed)
        want_tx, want_sym = synth.make_frames_philox_numpy(code, pc, F, L, 3.0, seed=seed)
        got[seed] = (tx.cpu().numpy(), sym.cpu().numpy())
        assert np.array_equal(got[seed][0], want_tx), seed
        _close_to_the_mirror(("seed", seed), got[seed][1], want_sym)
    # 1 and 2^63 + 1 share the low word
    assert not np.array_equal(got[1][0], got[(1 << 63) + 1][0]) and not np.array_equal(got[1][1], got[(1 << 63) + 1][1])
    assert not np.array_equal(got[1][0], got[1 << 32][0])


PLACED = [(1, "SOFT8"), (1, "SOFT16"), (2, "SOFT8"), (2, "SOFT16"), (3, "HARD8"), (3, "SOFT16")]


def _placed_decoder(R, decode_type):
    if R == 1:
        return extra_decoder("R1", decode_type)
    code = COMMON_CODES[R]                      # Voyager, LTE
    pc, table, config = make_table_config(code, decode_type)
    return code, pc, BatchDecoder(table, config)


@pytest.mark.parametrize("R,decode_type", PLACED)
def test_store_paths_guard_bands_and_a_null_tx(R, decode_type):
    """the symbols at the base offsets that select the 16-, 8- and 4-byte and the scalar store (int8: 0, 1, 2, 4, 8 bytes behind a
    16-byte boundary; int16: 0, 2, 4, 8), tx at an odd address, both inside poisoned buffers with 64-byte guards compared whole; and
    d_tx_bytes == NULL gives the same symbols"""
    import torch
    code, pc, dec = _placed_decoder(R, decode_type)
    width = pc.soft_bytes
    F, L = 3, 40                                # S = L + K - 1 ends inside a chunk of 8 steps: the last chunk of a frame is ragged
    S = L + code.K - 1
    assert S % 8 != 0
    want_tx, want_sym = synth.make_frames_philox_numpy(code, pc, F, L, None, seed=5, first_frame=2)
    nsym, ntx = F * S * code.R * width, F * L // 8
    for off in ((0, 1, 2, 4, 8) if width == 1 else (0, 2, 4, 8)):
        for with_tx in (True, False):
            symbuf = torch.full((GUARD + off + nsym + GUARD,), POISON, dtype=torch.uint8, device="cuda")
            txbuf = torch.full((GUARD + 1 + ntx + GUARD,), POISON, dtype=torch.uint8, device="cuda")
            assert symbuf.data_ptr() % 16 == 0
            rc = synth_raw(dec, F, L, seed=5, first_frame=2, tx=txbuf.data_ptr() + GUARD + 1 if with_tx else None,
                           sym=symbuf.data_ptr() + GUARD + off)
            assert rc == _lib.OK, (off, with_tx)
            want = np.full(symbuf.numel(), POISON, dtype=np.uint8)
            want[GUARD + off:GUARD + off + nsym] = want_sym.reshape(-1).view(np.uint8)
            got = symbuf.cpu().numpy()
            assert np.array_equal(got, want), (off, with_tx, np.argwhere(got != want)[:4].tolist())
            want = np.full(txbuf.numel(), POISON, dtype=np.uint8)
            if with_tx:
                want[GUARD + 1:GUARD + 1 + ntx] = want_tx.reshape(-1)
            assert np.array_equal(txbuf.cpu().numpy(), want), (off, with_tx)


@pytest.mark.parametrize("name,decode_type,ebn0", [("R1", "SOFT16", 4.0), (3, "SOFT16", 1.0), ("R5", "SOFT16", 0.0)], ids=str)
def test_noisy_frames_of_rates_1_3_and_5_follow_the_mirror(name, decode_type, ebn0):
    if isinstance(name, int):
        code = COMMON_CODES[name]
        pc, table, config = make_table_config(code, decode_type)
        dec = BatchDecoder(table, config)
    else:
        code, pc, dec = extra_decoder(name, decode_type)
    F, L = 8, 512
    tx, sym = dec.synth(F, L, ebn0, seed=314)
    want_tx, want_sym = synth.make_frames_philox_numpy(code, pc, F, L, ebn0, seed=314)
    assert np.array_equal(tx.cpu().numpy(), want_tx)
    sym = sym.cpu().numpy()
    _close_to_the_mirror((code.name, ebn0), sym, want_sym)
    assert sym.max() <= pc.soft_decision_high and sym.min() >= pc.soft_decision_low
    assert len(np.unique(sym)) > 50                                            # noise, not the two levels


def test_synth_rejections_leave_the_outputs_untouched():
    import torch
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    F, L = 3, 16
    sym = torch.full((F * (L + code.K - 1) * code.R + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
    tx = torch.full((F * L // 8 + 8,), POISON, dtype=torch.uint8, device="cuda")
    BAD = _lib.ERR_INVALID_ARG
    assert synth_raw(dec, F, 12, tx=tx.data_ptr(), sym=sym.data_ptr()) == BAD
    assert synth_raw(dec, F, L, tx=tx.data_ptr(), sym=sym.data_ptr() + 1) == BAD
    assert synth_raw(dec, F, L, tx=tx.data_ptr(), sym=None) == BAD
    assert _lib.load().vit_hip_synth_batch(None, F, L, 1, 0, 0.0, 1, tx.data_ptr(), sym.data_ptr(), None) == BAD
    # a two-valued table that is no convolutional code's
    odd_table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    odd_table._table[0, 5] = pc.soft_decision_high + pc.soft_decision_low - odd_table._table[0, 5]
    odd = BatchDecoder(odd_table, ViterbiDecoder_Config.from_decoder_config(pc))
    assert odd._handle.info.table_is_linear == 0
    assert synth_raw(odd, F, L, tx=tx.data_ptr(), sym=sym.data_ptr()) == _lib.ERR_UNSUPPORTED
    assert synth_raw(dec, 0, L, tx=tx.data_ptr(), sym=sym.data_ptr()) == _lib.OK
    assert synth_raw(dec, 0, 12, tx=None, sym=None) == _lib.OK
    assert (sym == 0x5A5A).all() and (tx == POISON).all()
    # the same buffers take a good call: an odd address is legal for 8-bit symbols, here the int16 call at the even one writes
    assert synth_raw(dec, F, L, tx=tx.data_ptr(), sym=sym.data_ptr()) == _lib.OK
    assert not (sym[:-8] == 0x5A5A).any() and (sym[-8:] == 0x5A5A).all() and (tx[-8:] == POISON).all()
