"""The hypothesis sets of node synchronisation (BatchDecoder.sync_search / vit_hip_sync_search).

A hypothesis is (offset, flags): offset = received symbols in front of the first symbol of a puncturing period -- 0 .. kept_per_period-1
covers the symbol alignment within a trellis step and the puncture phase at once (unpunctured: kept_per_period = R) --, flags a set of
_lib.SYNC_SWAP_PAIRS (I <-> Q), SYNC_NEGATE_EVEN (I mirrored), SYNC_NEGATE_ODD (Q mirrored).
"""
from __future__ import annotations

from . import _lib

SWAP, NEG_EVEN, NEG_ODD = _lib.SYNC_SWAP_PAIRS, _lib.SYNC_NEGATE_EVEN, _lib.SYNC_NEGATE_ODD

# what the carrier loop may have settled in, upright first: on a transparent code the inverted stream ties with the upright one and the
# search names the lower index
ROTATIONS = {
    "none": (0,),
    "bpsk": (0, NEG_EVEN | NEG_ODD),
    "qpsk": (0, SWAP | NEG_EVEN, NEG_EVEN | NEG_ODD, SWAP | NEG_ODD),
}


def enumerate_hypotheses(kept_per_period: int, rotations: str = "none"):
    """[(offset, flags)] for every offset 0 .. kept_per_period-1 and every rotation of the set "none", "bpsk" or "qpsk", offset-major"""
    if rotations not in ROTATIONS:
        raise ValueError(f"rotations must be one of {sorted(ROTATIONS)}")
    kept_per_period = int(kept_per_period)
    if kept_per_period < 1:
        raise ValueError("kept_per_period must be >= 1")
    return [(offset, flags) for offset in range(kept_per_period) for flags in ROTATIONS[rotations]]
