"""The host mirror of the device frame generator against what is published: synth.philox4x32_10 gives the known-answer vectors of
Random123 (Salmon et al., SC'11: kat_vectors, philox4x32 with 10 rounds).  tests/test_gpu_synth.py holds the device to the mirror, so
the two together tie the device generator to the published one.  No GPU."""
import numpy as np
import pytest

from viterbidecodercpp_amd import synth


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
], ids=["zeros", "ones", "pi"])
def test_philox4x32_10_known_answers(ctr, key, want):
    got = synth.philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in got) == want


def test_philox_broadcasts_and_the_counter_words_are_independent():
    """arrays give what scalars give element by element; every counter word and both key words change the block"""
    c = np.array([0x243f6a88, 0, 7], dtype=np.uint64)
    got = np.stack(synth.philox4x32_10(c, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0), axis=-1)
    for i, c0 in enumerate(c.tolist()):
        assert got[i].tolist() == [int(x) for x in synth.philox4x32_10(c0, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)]
    base = [int(x) for x in synth.philox4x32_10(1, 2, 3, 4, 5, 6)]
    for word in range(6):
        args = [1, 2, 3, 4, 5, 6]
        args[word] += 1
        assert [int(x) for x in synth.philox4x32_10(*args)] != base


def test_info_bytes_take_the_frame_and_seed_words_apart():
    """philox_info_bytes: first_frame above 2^32 reaches the high counter word, a seed above 2^32 the second key word"""
    a = synth.philox_info_bytes(2, 16, seed=(7 << 32) | 9, first_frame=(1 << 32) + 5)
    want = np.stack(synth.philox4x32_10(0, np.array([5, 6]), 0, 1, 9, 7), axis=-1).astype("<u4")
    assert np.array_equal(a, want.view(np.uint8).reshape(2, 16))
