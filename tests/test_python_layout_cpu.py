"""The Python layer's layout: the public surface of BatchDecoder, MultiStreamDecoder and StreamDecoder is what it was before the host
layer was split into _args.py (the tensor rules), outer.py (the outer chain) and the receiver's _FrameChain -- every public name with
its signature, recorded below --, and each tensor rule of _args.py turns down a CPU tensor, a wrong dtype and a tensor that is not
contiguous with ValueError.  No GPU."""
import inspect

import pytest
import torch

from viterbidecodercpp_amd import BatchDecoder, MultiStreamDecoder, StreamDecoder, _args

PARENT_SIGNATURES = {
    "BatchDecoder": {
        "__init__": "(self, branch_table: 'ViterbiBranchTable' = None, config: 'ViterbiDecoder_Config' = None, device=0, blob: 'bytes' = None, plan: 'int' = 0)",
        "chainback": "(self, frames: 'int', L: 'int', end_state=None, out=None, workspace=None, kernel=None)",
        "channel_errors": "(self, symbols, bytes, L: 'int', tail=True, tail_biting=False, start_state=None, symbol_frame_stride: 'int' = 0, bytes_frame_stride: 'int' = 0)",
        "count_bit_errors": "(self, a, b, count=None)",
        "decode": "(self, symbols, L: 'int', out=None, want_metrics=False)",
        "decode_stream": "(self, symbols, begin=True, end=False, window: 'int' = None, head: 'int' = None, tail: 'int' = None, out=None, workspace=None)",
        "decode_streams": "(self, symbols, steps: 'int' = None, begin=True, end=False, window: 'int' = None, head: 'int' = None, tail: 'int' = None, out=None, workspace=None)",
        "decode_tail_biting": "(self, symbols, L: 'int', head: 'int' = None, tail: 'int' = None, out=None, end_state_out=None, ok_out=None, workspace=None)",
        "deinterleave": "(self, packets, n_frames=None, branches: 'int' = 12, cell: 'int' = 17, hist=None, fill=None, packet_bytes: 'int' = None, out=None)",
        "depuncture": "(self, punctured, mask, out=None)",
        "dvb_derandomize": "(self, packets, n_frames=None, phase=None, rs_status=None, out=None, phase_out=None, sync_errors=None, in_place: 'bool' = False)",
        "encode": "(self, bytes, L: 'int', tail=True, tail_biting=False, start_state=None, out=None, end_state_out=False)",
        "export_decisions": "(self, frames: 'int', L: 'int', n_steps: 'int' = None, workspace=None, first_frame: 'int' = 0)",
        "frames_capacity": "(self, n_bits: 'int', period: 'int') -> 'int'",
        "frames_extract": "(self, bytes, n_bits: 'int', period: 'int', phase0: 'int', lock, carry=None, carry_bits=None, marker: 'int' = 0, marker_bits: 'int' = 0, drop_bits: 'int' = 0, pad=None, max_frames: 'int' = None, out=None)",
        "kernel_resources": "(self, kernel: 'int' = 0) -> 'dict'",
        "marker_search": "(self, bytes, n_bits: 'int', marker: 'int', marker_bits: 'int', period: 'int', phase0: 'int' = 0, history=None, history_bits: 'int' = 0, out=None, accumulate=False)",
        "new_workspace": "(self, frames: 'int', L: 'int')",
        "plan": "property",
        "plan_note": "property",
        "reset_batch": "(self, frames: 'int', start_state=None, metrics_out=None)",
        "rs_decode": "(self, code, frames, n_frames=None, interleave: 'int' = 1, out=None, status=None)",
        "set_plan": "(self, plan: 'int')",
        "stream_workspace_bytes": "(self, steps: 'int', begin=True, end=False, window: 'int' = None, head: 'int' = None, tail: 'int' = None) -> 'int'",
        "streams_workspace_bytes": "(self, n_streams: 'int', pitch: 'int', steps: 'int', begin=True, end=False, window: 'int' = None, head: 'int' = None, tail: 'int' = None) -> 'int'",
        "sync_build": "(self, received, hypotheses, steps: 'int', mask=None, pitch: 'int' = None, out=None)",
        "sync_search": "(self, received, hypotheses, steps: 'int', mask=None, window: 'int' = None, head: 'int' = None, tail: 'int' = None, workspace=None)",
        "sync_search_workspace_bytes": "(self, n_hyp: 'int', steps: 'int', window: 'int' = None, head: 'int' = None, tail: 'int' = None) -> 'int'",
        "synth": "(self, frames: 'int', L: 'int', ebn0_db, seed: 'int' = 1, first_frame: 'int' = 0, tx_out=None, symbols_out=None)",
        "tail_biting_workspace_bytes": "(self, frames: 'int', L: 'int', head: 'int' = None, tail: 'int' = None) -> 'int'",
        "update": "(self, symbols, L: 'int', n_steps: 'int' = None, start_state=None, want_metrics=True, metrics_out=None, renorm_out=None, workspace=None)",
        "update_resume": "(self, symbols, L: 'int', first_step: 'int', metrics, n_steps: 'int' = None, symbol_frame_stride: 'int' = 0, renorm_out=None, workspace=None)",
        "workspace_bytes": "(self, frames: 'int', L: 'int') -> 'int'",
    },
    "MultiStreamDecoder": {
        "__init__": "(self, decoder: 'BatchDecoder', n_streams: 'int', window: 'int' = None, head: 'int' = None, tail: 'int' = None, channel_errors: 'bool' = False, marker=None, period: 'int' = None, frames: 'bool' = False, frame_drop_bits: 'int' = 0, frame_pad=None, rs=None, rs_interleave: 'int' = 1, deinterleave=None, dvb_derandomize: 'bool' = False)",
        "channel_errors": "property",
        "finish": "(self, symbols=None) -> 'list'",
        "marker_lock": "property",
        "marker_totals": "property",
        "push": "(self, symbols) -> 'list'",
        "take_frames": "(self) -> 'list'",
    },
    "StreamDecoder": {
        "__init__": "(self, decoder: 'BatchDecoder', window: 'int' = None, head: 'int' = None, tail: 'int' = None, channel_errors: 'bool' = False, marker=None, period: 'int' = None, frames: 'bool' = False, frame_drop_bits: 'int' = 0, frame_pad=None, rs=None, rs_interleave: 'int' = 1, deinterleave=None, dvb_derandomize: 'bool' = False)",
        "channel_errors": "property",
        "finish": "(self, symbols=None) -> 'bytes'",
        "marker_lock": "property",
        "marker_totals": "property",
        "push": "(self, symbols) -> 'bytes'",
        "take_frames": "(self)",
    },
}

CLASSES = {"BatchDecoder": BatchDecoder, "MultiStreamDecoder": MultiStreamDecoder, "StreamDecoder": StreamDecoder}


@pytest.mark.parametrize("cls", sorted(PARENT_SIGNATURES))
def test_every_public_name_keeps_its_signature(cls):
    for name, want in PARENT_SIGNATURES[cls].items():
        attr = inspect.getattr_static(CLASSES[cls], name)
        if want == "property":
            assert isinstance(attr, property), (cls, name)
        else:
            assert str(inspect.signature(getattr(CLASSES[cls], name))) == want, (cls, name)


def test_the_names_others_reach_into_stay():
    from viterbidecodercpp_amd.decoder import DecodePipeline                  # noqa: F401
    from viterbidecodercpp_amd.outer import _OuterChain
    assert issubclass(BatchDecoder, _OuterChain)
    for name in ("_stream", "_rs_code", "_stream_args", "_check_symbols"):
        assert callable(getattr(BatchDecoder, name)), name
    for name in ("marker_search", "frames_capacity", "frames_extract", "rs_decode", "deinterleave", "dvb_derandomize", "_rs_code"):
        assert name in vars(_OuterChain) and name not in vars(BatchDecoder), name


U8, I32 = torch.uint8, torch.int32
# (rule, the call on a tensor x, the shape and dtype of an x that only the device is wrong with)
RULES = [
    ("device", lambda x: _args.device(x, U8, "x"), (4, 6), U8),
    ("dense", lambda x: _args.dense(x, I32, 24, "x"), (4, 6), I32),
    ("counts", lambda x: _args.counts(x, 4, "x"), (4,), I32),
    ("bit_rows", lambda x: _args.bit_rows(x, 48), (4, 6), U8),
    ("packets", lambda x: _args.packets(x, "x", 6), (2, 4, 6), U8),
    ("row_buffer", lambda x: _args.row_buffer(x, 4, 6, "x"), (4, 6), U8),
    ("carried-next", lambda x: _args.carried(None, None, x, 4, 6, "x", "n"), (4, 6), U8),
]


@pytest.mark.parametrize("rule,call,shape,dtype", RULES, ids=[r[0] for r in RULES])
def test_each_rule_turns_down_cpu_dtype_and_strides(rule, call, shape, dtype):
    good = torch.zeros(shape, dtype=dtype)
    strided = torch.zeros(shape + (2,), dtype=dtype)[..., 0]
    assert not strided.is_contiguous() and strided.shape == good.shape
    for x in (good, good.to(torch.int64), strided):
        with pytest.raises(ValueError, match="bytes" if rule == "bit_rows" else "x"):
            call(x)


def test_rules_without_a_tensor_of_their_own():
    assert _args.counts(None, 4, "x") is None and _args.state_tensor(torch, "cpu", None) is None
    assert _args.state_tensor(torch, "cpu", [[1], [2]], 2).tolist() == [1, 2]
    with pytest.raises(ValueError, match="start_state"):
        _args.state_tensor(torch, "cpu", [1, 2, 3], 2)
