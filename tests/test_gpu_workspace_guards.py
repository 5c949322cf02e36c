"""The caller-owned workspaces of the windowed decodes (csrc/vit_windows.hip: tail-biting, one stream, many streams), exactly as
large as the *_workspace_bytes functions say and cut out of a larger poisoned buffer: the results equal the references and the 256
bytes in front of and behind the workspace are untouched.  The shapes are the smallest at which a misplaced part of the layout
shows: at K = 3 SOFT8 a metrics row is 4 bytes, so every part is mostly padding and a part that starts one slot early lands on its
neighbour's data; with a remainder window both halves of the stream layout exist, without one (and with nothing but remainder
windows, rows_u == 0) the conditional parts are empty.  The workspace of a synchronisation search (csrc/vit_sync.hip) carves the
hypothesis streams, their decoded bytes and the start states in front of a decode_streams workspace: 64 hypotheses make it as large as
it gets, an int8 search with rows of 300 bytes makes every part mostly padding."""
import ctypes as C

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, _lib
from tests import sync_reference
from tests.helpers import make_table_config, oracle_cfg, sync_search_raw
from tests.stream_reference import BEGIN, END, default_extension, make_stream, stream_reference
from tests.tb_reference import tb_frames, tb_reference

pytestmark = pytest.mark.gpu

GUARD, POISON, W = 256, 0xA5, 64
ROUTES = ["tail_biting", "stream_remainder", "stream_uniform", "streams_remainder", "streams_no_grid"]


class GuardedWorkspace:
    """`need` bytes, 256-byte aligned, with GUARD poisoned bytes either side"""

    def __init__(self, need):
        import torch

        assert need > 0 and need % 256 == 0
        self.need = need
        self.buf = torch.full((GUARD + need + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 256 == 0

    def guards_intact(self):
        host = self.buf.cpu().numpy()
        return bool(np.all(host[:GUARD] == POISON)), bool(np.all(host[GUARD + self.need:] == POISON))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("code,decode_type", [(COMMON_CODES[0], "SOFT8"), (COMMON_CODES[2], "SOFT16")], ids=["K3-soft8", "K7-soft16"])
def test_exact_workspace_between_guards(oracle, code, decode_type, route):
    import torch

    pc, table, config = make_table_config(code, decode_type)
    ocfg = oracle_cfg(decode_type, code.R)
    dec = BatchDecoder(table, config)
    lib, h = _lib.load(), dec._handle._h
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    d = default_extension(code.K)
    assert d <= W
    tag = (code.name, decode_type, route)

    if route == "tail_biting":
        F, L = 3, 40
        _, sym = tb_frames(code, pc, F, L, 3.0, seed=code.K)
        want_out, want_ends, want_ok = tb_reference(oracle, code, ocfg, sym, L, d, d)
        ws = GuardedWorkspace(lib.vit_hip_tail_biting_workspace_bytes(h, F, L, d, d))
        d_sym = torch.from_numpy(sym).cuda()
        out = torch.full(want_out.shape, POISON, dtype=torch.uint8, device="cuda")
        ends = torch.full((F,), -1, dtype=torch.int32, device="cuda")
        ok = torch.full((F,), POISON, dtype=torch.uint8, device="cuda")
        rc = lib.vit_hip_decode_tail_biting_batch(h, p(d_sym), F, L, d, d, C.c_void_p(ws.ptr), ws.need, p(out), p(ends), p(ok), stream)
        assert rc == _lib.OK, (tag, lib.vit_hip_last_error())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want_out), tag
        assert np.array_equal(ends.cpu().numpy().view(np.uint32), want_ends), tag
        assert np.array_equal(ok.cpu().numpy(), want_ok), tag
    else:
        # (n_streams, T, flags): two grid windows and a longer third one; the same without it; three streams of that shape; three
        # streams that are one window of their own length each
        ns, T, flags = {"stream_remainder": (1, d + 2 * W + d + 5, 0), "stream_uniform": (1, d + 2 * W + d, BEGIN),
                        "streams_remainder": (3, d + 2 * W + d + 5, BEGIN | END), "streams_no_grid": (3, d + d + 9, BEGIN | END)}[route]
        pitch = 4 * W if route == "streams_remainder" else -(-T // W) * W
        streams = [make_stream(code, pc, T + 40, 3.0, seed=10 * code.K + s)[1][(0 if flags & BEGIN else 7):][:T] for s in range(ns)]
        want = [stream_reference(oracle, code, ocfg, s, W, d, d, flags) for s in streams]
        nb, want_n = want[0][0].size, want[0][1]
        buf = np.zeros(((ns - 1) * pitch + T, code.R), dtype=streams[0].dtype)
        for s, sym in enumerate(streams):
            buf[s * pitch:s * pitch + T] = sym
        d_buf = torch.from_numpy(buf).cuda()
        out = torch.full((ns, nb), POISON, dtype=torch.uint8, device="cuda")
        n_bits = C.c_size_t(0)
        if route.startswith("streams"):
            ws = GuardedWorkspace(lib.vit_hip_streams_workspace_bytes(h, ns, pitch, T, W, d, d, flags))
            rc = lib.vit_hip_decode_streams(h, p(d_buf), ns, pitch, T, W, d, d, flags, C.c_void_p(ws.ptr), ws.need, p(out), nb,
                                            C.byref(n_bits), stream)
        else:
            ws = GuardedWorkspace(lib.vit_hip_stream_workspace_bytes(h, T, W, d, d, flags))
            rc = lib.vit_hip_decode_stream(h, p(d_buf), T, W, d, d, flags, C.c_void_p(ws.ptr), ws.need, p(out), C.byref(n_bits), stream)
        assert rc == _lib.OK, (tag, lib.vit_hip_last_error())
        torch.cuda.synchronize()
        assert n_bits.value == want_n, tag
        assert np.array_equal(out.cpu().numpy(), np.stack([w[0] for w in want])), tag
    assert ws.guards_intact() == (True, True), f"{tag}: wrote in front of / behind its workspace"


@pytest.mark.parametrize("name", ["voyager_64", "voy_soft8", "lte_soft8_head15"])
def test_exact_sync_search_workspace_between_guards(oracle, name):
    import torch

    c = sync_reference.make_case(name)
    want_err, want_cmp, want_best, _ = sync_reference.case_reference(oracle, name)
    pc, table, config = make_table_config(c["code"], c["decode_type"])
    dec = BatchDecoder(table, config)
    n = len(c["hypotheses"])
    ws = GuardedWorkspace(_lib.load().vit_hip_sync_search_workspace_bytes(dec._handle._h, n, c["T"], c["W"], c["head"], c["tail"]))
    out = torch.full((3, 64), -1, dtype=torch.int32, device="cuda")
    rc = sync_search_raw(dec, c, ws.ptr, ws.need, out[0], out[1], out[2])
    assert rc == _lib.OK, (name, _lib.load().vit_hip_last_error())
    host = out.cpu().numpy()
    assert host[0, :n].tolist() == want_err.tolist() and host[1, :n].tolist() == want_cmp.tolist() and int(host[2, 0]) == want_best, name
    assert (host[:2, n:] == -1).all() and (host[2, 1:] == -1).all(), name
    assert ws.guards_intact() == (True, True), f"{name}: wrote in front of / behind its workspace"
