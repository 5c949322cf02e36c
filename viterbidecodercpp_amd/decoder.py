"""Host-side mirror of the reference's decoder interface, over the C ABI (include/vit_hip.h).

Names, argument meaning and call pattern follow the reference so that tests read like its own:

    table  = ViterbiBranchTable(K, R, G, soft_decision_high, soft_decision_low, soft_dtype)   # viterbi_branch_table.h:34
    vitdec = ViterbiDecoder_Core(table, config)                                               # viterbi_decoder_core.h:170
    vitdec.set_traceback_length(total_input_bits); vitdec.reset()                             # :180, :202
    acc = ViterbiDecoder_HIP.update(vitdec, symbols)                                          # viterbi_decoder_scalar.h:29
    err = acc + vitdec.get_error(); data = vitdec.chainback(total_input_bits)                 # core.h:195, :214

`ViterbiDecoder_HIP` is the GPU decoder strategy (the counterpart of ViterbiDecoder_Scalar / _AVX_u16 ...): update() and
chainback() run as HIP kernels on gfx950; nothing here decodes on the CPU.  `BatchDecoder` is the throughput route:
many independent frames, device-resident tensors, explicit stream.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _args, _lib
from .codes import DecoderConfig
from .outer import _OuterChain, _ptr


def _parity(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    x ^= x >> 16
    x ^= x >> 8
    x ^= x >> 4
    x ^= x >> 2
    x ^= x >> 1
    return (x & 1).astype(np.uint8)


class ViterbiBranchTable:
    """Expected symbol value for each half-state and polynomial: bt[i][s] = parity((s << 1) & G[i]) ? high : low
    (include/viterbi/viterbi_branch_table.h:44-54).  Shareable between decoders (README.md:14)."""

    def __init__(self, K: int, R: int, G, soft_decision_high: int, soft_decision_low: int, soft_dtype=np.int16):
        if K < 2 or R < 1:
            raise ValueError("K >= 2 and R >= 1 required")
        if len(G) != R:
            raise ValueError("need exactly R polynomials")
        if not soft_decision_high > soft_decision_low:
            raise ValueError("soft_decision_high must exceed soft_decision_low")
        self.K, self.R, self.G = K, R, tuple(int(g) for g in G)
        self.soft_decision_high, self.soft_decision_low = int(soft_decision_high), int(soft_decision_low)
        self.soft_dtype = np.dtype(soft_dtype)
        self.NUMSTATES = max((1 << (K - 1)) // 2, 1)
        s = np.arange(self.NUMSTATES, dtype=np.uint32) << 1
        rows = [np.where(_parity(s & np.uint32(g)) != 0, self.soft_decision_high, self.soft_decision_low) for g in self.G]
        self._table = np.ascontiguousarray(np.stack(rows).astype(self.soft_dtype))

    def __getitem__(self, index):
        return self._table[index]

    def data(self) -> np.ndarray:
        return self._table


@dataclass
class ViterbiDecoder_Config:
    """include/viterbi/viterbi_decoder_config.h:11-18 (+ the error_t width)."""
    soft_decision_max_error: int
    initial_start_error: int
    initial_non_start_error: int
    renormalisation_threshold: int
    error_dtype: object = np.uint16

    @classmethod
    def from_decoder_config(cls, c: DecoderConfig):
        return cls(c.soft_decision_max_error, c.initial_start_error, c.initial_non_start_error,
                   c.renormalisation_threshold, c.error_dtype)

    def as_array(self):
        return np.asarray([self.soft_decision_max_error, self.initial_start_error, self.initial_non_start_error,
                           self.renormalisation_threshold], dtype=self.error_dtype)


class _Handle:
    def __init__(self, table: ViterbiBranchTable, config: ViterbiDecoder_Config, device: int = 0, blob: bytes = None):
        L = _lib.load()
        self._h = C.c_void_p()
        if blob is not None:
            buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
            _lib.check(L.vit_hip_create_from_blob(buf, len(blob), device, C.byref(self._h)))
        else:
            cfg = config.as_array()
            edt = np.dtype(config.error_dtype)
            if (table.soft_dtype.itemsize, edt.itemsize) not in ((2, 2), (1, 1)):
                raise ValueError("(soft_t, error_t) must be (int16, uint16) or (int8, uint8)")
            _lib.check(L.vit_hip_create(table.K, table.R, table.soft_dtype.itemsize, edt.itemsize,
                                        table.data().ctypes.data_as(C.c_void_p), cfg.ctypes.data_as(C.c_void_p), device,
                                        C.byref(self._h)))
        self.info = _lib.VitHipInfo()
        _lib.check(L.vit_hip_get_info(self._h, C.byref(self.info)))

    def refresh(self):
        _lib.check(_lib.load().vit_hip_get_info(self._h, C.byref(self.info)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().vit_hip_destroy(self._h)
                self._h = None
        except Exception:
            pass


def pack_blob(table: ViterbiBranchTable, config: ViterbiDecoder_Config) -> bytes:
    """table + config as the byte blob rank 0 broadcasts to the other GPUs (vit_hip_pack_blob)."""
    L = _lib.load()
    edt = np.dtype(config.error_dtype)
    n = L.vit_hip_blob_bytes(table.K, table.R, table.soft_dtype.itemsize, edt.itemsize)
    buf = (C.c_uint8 * n)()
    cfg = config.as_array()
    _lib.check(L.vit_hip_pack_blob(table.K, table.R, table.soft_dtype.itemsize, edt.itemsize,
                                   table.data().ctypes.data_as(C.c_void_p), cfg.ctypes.data_as(C.c_void_p), buf, n))
    return bytes(buf)


class ViterbiDecoder_Core:
    """Decoder state with the reference's public surface (viterbi_decoder_core.h:157-243): m_metrics, m_decisions and
    m_current_decoded_bit are host-visible; update() and chainback() execute on the GPU.

    Streamed update() calls (a few trellis steps each: examples/helpers/puncture_code_helpers.h:51 hands over ONE step per
    call) are queued on the host and run in one launch when the queue is full, when the cursor reaches the end of the traceback
    buffer, or when anything reads the state (m_metrics, m_decisions, get_error, chainback) -- the same scheme as the C++
    header include/viterbi_hip/viterbi_decoder_core.h ("deferred streaming")."""

    MAX_PENDING_STEPS = 2048
    MAX_DEFERRED_CALL_STEPS = 64

    def __init__(self, branch_table: ViterbiBranchTable, config: ViterbiDecoder_Config, device: int = 0):
        self.m_branch_table = branch_table
        self.m_config = config
        self.K, self.R = branch_table.K, branch_table.R
        self.TOTAL_STATE_BITS = self.K - 1
        self.NUMSTATES = 1 << (self.K - 1)
        self.TOTAL_BLOCKS = max(self.NUMSTATES // 64, 1)
        self._handle = _Handle(branch_table, config, device)
        self._metrics = np.zeros(self.NUMSTATES, dtype=config.error_dtype)
        self._decisions = np.zeros((0, self.TOTAL_BLOCKS), dtype=np.uint64)
        self._pending, self._pending_steps, self._unreported = [], 0, 0
        self._dropped = 0
        self._dev_begin = self._dev_end = 0     # rows [begin, end) of _decisions are stale here: they live in the handle's device row store
        self._exact_update_return = False
        self.m_current_decoded_bit = 0
        self.reset()
        self.set_traceback_length(0)

    # the public data members of the reference: reading them brings the decoder up to date first
    @property
    def m_metrics(self):
        self.flush_pending()
        return self._metrics

    @property
    def m_decisions(self):
        # the array handed out is writable: queued steps run, device-resident rows come home, the host copy is the authority again
        self.flush_pending()
        self.fetch_device_rows()
        return self._decisions

    def fetch_device_rows(self):
        """update() leaves the rows it computes in the handle's device row store (vit_hip_update_host_lazy); this copies the stale
        range back and makes the host rows authoritative (what reading m_decisions does)."""
        b, e = self._dev_begin, min(self._dev_end, len(self._decisions))
        self._dev_begin = self._dev_end = 0
        if e > b:
            rows = np.zeros((e - b, self.TOTAL_BLOCKS), dtype=np.uint64)
            _lib.check(_lib.load().vit_hip_fetch_decisions_host(self._handle._h, b, e - b, rows.ctypes.data_as(C.c_void_p)))
            self._decisions[b:e] = rows

    @property
    def rows_on_device(self) -> int:
        return self._dev_end - self._dev_begin

    def host_route_note(self) -> str:
        """vit_hip_host_route_note: the kernel family behind this object's update() / chainback(), in one line"""
        return _lib.load().vit_hip_host_route_note(self._handle._h).decode()

    def set_host_route(self, route: int):
        """_lib.HOST_ROUTE_LDS puts the general LDS plan behind update() / chainback() at any K (same results: an A/B inside one
        process); _lib.HOST_ROUTE_AUTO, the default, gives the choice back"""
        self.flush_pending()
        _lib.check(_lib.load().vit_hip_set_host_route(self._handle._h, route))

    def set_traceback_length(self, traceback_length: int):
        self.flush_pending()
        self.fetch_device_rows()
        new_length = traceback_length + self.TOTAL_STATE_BITS
        old = self._decisions
        self._decisions = np.zeros((new_length, self.TOTAL_BLOCKS), dtype=np.uint64)
        n = min(len(old), new_length)
        self._decisions[:n] = old[:n]
        if self.m_current_decoded_bit > new_length:
            self.m_current_decoded_bit = new_length

    def get_traceback_length(self) -> int:
        return len(self._decisions) - self.TOTAL_STATE_BITS

    def get_error(self, end_state: int = 0) -> int:
        assert end_state < self.NUMSTATES
        return int(self.m_metrics[end_state])

    def set_exact_update_return(self, exact: bool):
        """True: nothing is deferred -- every update() call runs at once and returns what the reference's update() returns for
        that call (one GPU launch per call); False (default): short calls are queued (see the class docstring)."""
        self.flush_pending()
        self._exact_update_return = bool(exact)

    def reset(self, starting_state: int = 0):
        # queued steps are run before the state is dropped (the reference has run them); a renormalisation sum no update() call has
        # returned yet is DROPPED: a frame's tail never inflates the next frame's total (collect it with
        # take_unreported_renormalisation() before reset(), or stream in exact mode)
        self.flush_pending()
        self._dropped, self._unreported = self._unreported, 0
        self.m_current_decoded_bit = 0
        self._metrics[:] = self.m_config.initial_non_start_error
        self._metrics[starting_state & (self.NUMSTATES - 1)] = self.m_config.initial_start_error

    def _run(self, symbols, steps, first_row):
        """one launch (vit_hip_update_host_lazy): the rows stay on the device; a call that completes the frame also chains it back for
        (traceback length, end state 0), so that the chainback() behind it costs a memcpy"""
        if self._dev_end > self._dev_begin and (first_row > self._dev_end or first_row + steps < self._dev_begin):
            self.fetch_device_rows()             # not adjacent to the device-resident range: one range only
        rs = C.c_uint64(0)
        _lib.check(_lib.load().vit_hip_update_host_lazy(self._handle._h, self._metrics.ctypes.data_as(C.c_void_p),
                                                        symbols.ctypes.data_as(C.c_void_p), steps, first_row,
                                                        self.get_traceback_length(), 0, C.byref(rs)))
        if self._dev_end == self._dev_begin:
            self._dev_begin, self._dev_end = first_row, first_row + steps
        else:
            self._dev_begin, self._dev_end = min(self._dev_begin, first_row), max(self._dev_end, first_row + steps)
        return int(rs.value)

    def enqueue_steps(self, symbols, steps):
        self._pending.append(symbols)
        self._pending_steps += steps
        self.m_current_decoded_bit += steps
        if self._exact_update_return or self._pending_steps >= self.MAX_PENDING_STEPS or self.m_current_decoded_bit >= len(self._decisions):
            self.flush_pending()

    def flush_pending(self):
        if not self._pending_steps:
            return
        steps, self._pending_steps = self._pending_steps, 0
        symbols = np.ascontiguousarray(np.concatenate(self._pending))
        self._pending = []
        self._unreported += self._run(symbols, steps, self.m_current_decoded_bit - steps)

    def take_unreported_renormalisation(self) -> int:
        v, self._unreported = self._unreported, 0
        return v

    def last_dropped_renormalisation(self) -> int:
        """what the last reset() dropped: a renormalisation sum that had been computed (by a flush) but that no update() call had
        returned and nobody had collected -- 0 unless a frame shorter than the traceback buffer was streamed in short calls"""
        return self._dropped

    def chainback(self, total_bits: int, end_state: int = 0) -> np.ndarray:
        assert self.get_traceback_length() >= total_bits
        assert self.m_current_decoded_bit - self.TOTAL_STATE_BITS >= total_bits
        assert end_state < self.NUMSTATES
        out = np.zeros((total_bits + 7) // 8, dtype=np.uint8)
        self.flush_pending()
        if self._dev_begin == 0 and self._dev_end >= total_bits + self.TOTAL_STATE_BITS:
            # every row the traceback reads is still on the device: nothing travels, and if the update that completed the frame
            # already decoded exactly these bits no kernel runs either
            _lib.check(_lib.load().vit_hip_chainback_host_lazy(self._handle._h, total_bits, end_state, out.ctypes.data_as(C.c_void_p)))
            return out
        rows = np.ascontiguousarray(self.m_decisions[:total_bits + self.TOTAL_STATE_BITS])
        _lib.check(_lib.load().vit_hip_chainback_host(self._handle._h, rows.ctypes.data_as(C.c_void_p), total_bits,
                                                      end_state, out.ctypes.data_as(C.c_void_p)))
        return out


class ViterbiDecoder_HIP:
    """The MI355X decoder strategy: same concept as ViterbiDecoder_Scalar (static update(), is_valid)."""
    is_valid = True

    @staticmethod
    def update(base: ViterbiDecoder_Core, symbols) -> int:
        """returns the renormalisation sum of the steps COMPUTED since the last value it returned (zero while short calls are
        queued, their whole sum from the call that runs them): the caller's running total is the reference's whenever nothing is
        queued -- in particular after the call that completes a frame."""
        symbols = np.ascontiguousarray(symbols, dtype=base.m_branch_table.soft_dtype).reshape(-1)
        N = symbols.size
        assert N % base.R == 0
        total_decoded_bits = N // base.R
        max_decoded_bits = base.get_traceback_length() + base.TOTAL_STATE_BITS
        assert total_decoded_bits + base.m_current_decoded_bit <= max_decoded_bits
        if total_decoded_bits == 0:
            return 0
        if total_decoded_bits <= base.MAX_DEFERRED_CALL_STEPS:
            base.enqueue_steps(symbols.copy(), total_decoded_bits)
            return base.take_unreported_renormalisation()
        base.flush_pending()
        rs = base._run(symbols, total_decoded_bits, base.m_current_decoded_bit)
        base.m_current_decoded_bit += total_decoded_bits
        return rs + base.take_unreported_renormalisation()


class BatchDecoder(_OuterChain):
    """Frame-parallel decoder on device-resident torch tensors (vit_hip_*_batch).  torch is plumbing only: it owns the
    HBM buffers and the stream.  The outer chain behind the decoder (marker_search, frames_extract, rs_decode, deinterleave,
    dvb_derandomize) is mixed in from outer.py; the tensor rules of every method are those of _args.py."""

    def __init__(self, branch_table: ViterbiBranchTable = None, config: ViterbiDecoder_Config = None, device=0,
                 blob: bytes = None, plan: int = _lib.PLAN_AUTO):
        import torch

        self.torch = torch
        self.device_index = device if isinstance(device, int) else torch.device(device).index or 0
        self.device = torch.device("cuda", self.device_index)
        self._handle = _Handle(branch_table, config, self.device_index, blob=blob)
        if plan != _lib.PLAN_AUTO:
            self.set_plan(plan)
        i = self._handle.info
        self.K, self.R, self.N, self.W = i.K, i.R, i.num_states, i.decision_words
        self.soft_bytes, self.error_bytes = i.soft_bytes, i.error_bytes
        self._soft_dtype = torch.int16 if self.soft_bytes == 2 else torch.int8
        self._error_dtype = torch.int16 if self.error_bytes == 2 else torch.uint8     # int16 carries the uint16 bit pattern
        self._ws = None
        self._rs_codes = {}                     # RSCode -> _RsCode: a code's tables are uploaded once per decoder

    @property
    def plan(self) -> int:
        return self._handle.info.plan

    def set_plan(self, plan: int):
        _lib.check(_lib.load().vit_hip_set_plan(self._handle._h, plan))
        self._handle.refresh()

    @property
    def plan_note(self) -> str:
        """vit_hip_plan_note: which plan runs and, where that is the slow compatibility plan, whether a faster one exists"""
        return _lib.load().vit_hip_plan_note(self._handle._h).decode()

    def workspace_bytes(self, frames: int, L: int) -> int:
        return _lib.load().vit_hip_workspace_bytes(self._handle._h, frames, L)

    def _workspace(self, frames, L, workspace=None):
        return self._scratch(self.workspace_bytes(frames, L), workspace)

    def _scratch(self, need, workspace=None):
        """the caller's workspace once it has passed the size and alignment check, else the decoder's own, grown to `need` bytes"""
        if workspace is not None:
            if workspace.numel() * workspace.element_size() < need or workspace.data_ptr() % 256 != 0:
                raise ValueError("workspace too small or not 256-byte aligned")
            return workspace
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = self.torch.empty(need, dtype=self.torch.uint8, device=self.device)
        assert self._ws.data_ptr() % 256 == 0
        return self._ws

    def kernel_resources(self, kernel: int = 0) -> dict:
        """what one wave / workgroup of this decoder's kernel allocates, from its kernel descriptor (vit_hip_get_kernel_resources;
        kernel: _lib.KERNEL_UPDATE / _CHAINBACK / _CHAINBACK_ALT / _RESUME)"""
        r = _lib.VitHipKernelResources()
        _lib.check(_lib.load().vit_hip_get_kernel_resources(self._handle._h, int(kernel), C.byref(r)))
        return _lib._resources_dict(r)

    def new_workspace(self, frames: int, L: int):
        """a private decision workspace (for double-buffered pipelines: update of batch i+1 beside chainback of batch i)."""
        return self.torch.empty(self.workspace_bytes(frames, L), dtype=self.torch.uint8, device=self.device)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _check_symbols(self, symbols, n_steps):
        frames = _args.dense(symbols, self._soft_dtype, None, "symbols").shape[0]
        if symbols.numel() != frames * n_steps * self.R:
            raise ValueError("symbols must have shape [frames][n_steps][R]")
        return frames

    def update(self, symbols, L: int, n_steps: int = None, start_state=None, want_metrics=True, metrics_out=None,
               renorm_out=None, workspace=None):
        """reset + update over n_steps (default L+K-1) steps.  returns (final_metrics [F][N], renorm_sum [F]);
        with want_metrics=False and no *_out buffers nothing but the decision workspace is written."""
        t = self.torch
        n_steps = (L + self.K - 1) if n_steps is None else n_steps
        frames = self._check_symbols(symbols, n_steps)
        ws = self._workspace(frames, L, workspace)
        met, rs = metrics_out, renorm_out
        if want_metrics:
            met = t.empty((frames, self.N), dtype=self._error_dtype, device=self.device) if met is None else met
            rs = t.empty(frames, dtype=t.int64, device=self.device) if rs is None else rs
        ss = _args.state_tensor(t, self.device, start_state)
        _lib.check(_lib.load().vit_hip_update_batch(
            self._handle._h, _ptr(symbols), frames, n_steps, L, _ptr(ws), ws.numel() * ws.element_size(), _ptr(met), _ptr(rs), _ptr(ss),
            self._stream()))
        return met, rs

    def reset_batch(self, frames: int, start_state=None, metrics_out=None):
        """ViterbiDecoder_Core::reset for every frame (core.h:202-211): the device-resident metrics [F][N] a streamed decode
        starts from."""
        t = self.torch
        met = t.empty((frames, self.N), dtype=self._error_dtype, device=self.device) if metrics_out is None else metrics_out
        ss = _args.state_tensor(t, self.device, start_state)
        _lib.check(_lib.load().vit_hip_reset_batch(self._handle._h, frames, _ptr(ss), _ptr(met), self._stream()))
        return met

    def update_resume(self, symbols, L: int, first_step: int, metrics, n_steps: int = None, symbol_frame_stride: int = 0,
                      renorm_out=None, workspace=None):
        """update() on decoders that already hold state (no reset): consumes `n_steps` more trellis steps of every frame from
        cursor `first_step`, metrics [F][N] updated in place, decision rows [first_step, first_step + n_steps) written.
        `symbols` holds each frame's chunk [n_steps][R] -- either a [F][n_steps][R] tensor, or any tensor whose element
        `f * symbol_frame_stride` starts frame f's chunk (e.g. a view into the whole [F][S][R] batch).  returns renorm_sum [F]
        for THIS call."""
        t = self.torch
        frames = metrics.shape[0]
        if n_steps is None:
            n_steps = symbols.shape[1]
        if not _args.device(symbols, self._soft_dtype, "symbols").is_contiguous() and symbol_frame_stride == 0:
            raise ValueError("packed chunks must be contiguous (or pass symbol_frame_stride)")
        if metrics.dim() != 2 or metrics.shape[1] != self.N or not metrics.is_contiguous():
            raise ValueError("metrics must be a contiguous [frames][N] tensor")
        if symbol_frame_stride == 0 and symbols.dim() == 3 and (symbols.shape[0] != frames or symbols.shape[2] != self.R):
            raise ValueError("packed chunks must have shape [frames][n_steps][R]")
        # the kernels read frame f's chunk at f * stride: the tensor must cover the last frame's chunk
        stride = symbol_frame_stride or n_steps * self.R
        if frames and symbols.numel() < (frames - 1) * stride + n_steps * self.R:
            raise ValueError(f"symbols holds {symbols.numel()} elements; {frames} chunks of {n_steps} x {self.R} at stride "
                             f"{stride} need {(frames - 1) * stride + n_steps * self.R}")
        ws = self._workspace(frames, L, workspace)
        rs = t.empty(frames, dtype=t.int64, device=self.device) if renorm_out is None else renorm_out
        _lib.check(_lib.load().vit_hip_update_batch_resume(
            self._handle._h, _ptr(symbols), symbol_frame_stride, frames, first_step, n_steps, L, _ptr(ws), ws.numel() * ws.element_size(),
            _ptr(metrics), _ptr(rs), self._stream()))
        return rs

    def chainback(self, frames: int, L: int, end_state=None, out=None, workspace=None, kernel=None):
        """kernel: None (the code's stand-alone chainback kernel) or _lib.KERNEL_CHAINBACK / _lib.KERNEL_CHAINBACK_ALT
        (vit_hip_chainback_batch_ex: the other chainback kernel of the K = 7 / 9 register-plan codes; same results)"""
        t = self.torch
        ws = self._workspace(frames, L, workspace)
        if out is None:
            out = t.empty((frames, (L + 7) // 8), dtype=t.uint8, device=self.device)
        es = _args.state_tensor(t, self.device, end_state)
        if kernel is None:
            _lib.check(_lib.load().vit_hip_chainback_batch(self._handle._h, _ptr(ws), frames, L, _ptr(out), _ptr(es), self._stream()))
        else:
            _lib.check(_lib.load().vit_hip_chainback_batch_ex(self._handle._h, _ptr(ws), frames, L, _ptr(out), _ptr(es), self._stream(),
                                                              int(kernel)))
        return out

    def decode(self, symbols, L: int, out=None, want_metrics=False):
        """reset -> update -> chainback for every frame; returns bytes [F][L/8] (+ metrics, renorm when asked)."""
        t = self.torch
        frames = self._check_symbols(symbols, L + self.K - 1)
        ws = self._workspace(frames, L)
        if out is None:
            out = t.empty((frames, (L + 7) // 8), dtype=t.uint8, device=self.device)
        met = t.empty((frames, self.N), dtype=self._error_dtype, device=self.device) if want_metrics else None
        rs = t.empty(frames, dtype=t.int64, device=self.device) if want_metrics else None
        _lib.check(_lib.load().vit_hip_decode_batch(
            self._handle._h, _ptr(symbols), frames, L, _ptr(ws), ws.numel(), _ptr(out), _ptr(met), _ptr(rs), None, self._stream()))
        return (out, met, rs) if want_metrics else out

    def tail_biting_workspace_bytes(self, frames: int, L: int, head: int = None, tail: int = None) -> int:
        head, tail = self._tb_extension(head, tail)
        return _lib.load().vit_hip_tail_biting_workspace_bytes(self._handle._h, frames, L, head, tail)

    def _tb_extension(self, head, tail):
        d = 8 * (self.K - 1)                      # the default extension: byte-aligned, 48 steps at K = 7
        return (d if head is None else int(head)), (d if tail is None else int(tail))

    def decode_tail_biting(self, symbols, L: int, head: int = None, tail: int = None, out=None, end_state_out=None, ok_out=None,
                           workspace=None):
        """tail-biting frames (no tail; the encoder starts in the state the frame's last K-1 bits leave): symbols [F][L][R] ->
        bytes [F][ceil(L/8)] (vit_hip_decode_tail_biting_batch: wrap-around Viterbi with a fixed extension of `head` steps before
        and `tail` after the frame, default 8*(K-1) each).  end_state_out / ok_out: [F] int32 / uint8 device tensors, or True
        to have them allocated; either one asked for returns (bytes, end_state, ok), where ok[f] = 1 when the decoded path is a
        valid tail-biting codeword."""
        t = self.torch
        head, tail = self._tb_extension(head, tail)
        frames = self._check_symbols(symbols, L)
        need = self.tail_biting_workspace_bytes(frames, L, head, tail)
        if need == 0:
            raise ValueError(f"tail-biting decoding needs L >= K and head, tail >= K-1 (K = {self.K})")
        ws = self._scratch(need, workspace)
        if out is None:
            out = t.empty((frames, (L + 7) // 8), dtype=t.uint8, device=self.device)
        want_extra = end_state_out is not None or ok_out is not None
        if want_extra:
            if end_state_out is None or end_state_out is True:
                end_state_out = t.empty(frames, dtype=t.int32, device=self.device)
            if ok_out is None or ok_out is True:
                ok_out = t.empty(frames, dtype=t.uint8, device=self.device)
        for name, x, dt, n in (("out", out, t.uint8, frames * ((L + 7) // 8)), ("end_state_out", end_state_out, t.int32, frames),
                               ("ok_out", ok_out, t.uint8, frames)):
            if x is not None:
                _args.dense(x, dt, n, name)
        _lib.check(_lib.load().vit_hip_decode_tail_biting_batch(
            self._handle._h, _ptr(symbols), frames, L, head, tail, _ptr(ws), ws.numel() * ws.element_size(), _ptr(out), _ptr(end_state_out),
            _ptr(ok_out), self._stream()))
        return (out, end_state_out, ok_out) if want_extra else out

    def _stream_args(self, window, head, tail, begin, end):
        head, tail = self._tb_extension(head, tail)
        window = 1024 if window is None else int(window)
        return window, head, tail, (_lib.STREAM_BEGIN if begin else 0) | (_lib.STREAM_END if end else 0)

    def _emitted(self, T, head, tail, begin, end):
        """(a, b, bytes): a segment of T steps emits the bits of its steps [a, b), in ceil((b - a)/8) bytes"""
        a = 0 if begin else head
        b = T - (self.K - 1) if end else T - tail
        return a, b, (b - a + 7) // 8

    def _segment(self, need, workspace, T, head, tail, begin, end, rule):
        """what decode_stream and decode_streams share behind their symbol checks: the verdict of the argument rule (need = 0: outside
        it, `rule` says what it asks), the scratch workspace and the bytes one stream's segment emits"""
        if need == 0:
            raise ValueError(rule)
        return self._scratch(need, workspace), self._emitted(T, head, tail, begin, end)[2]

    def stream_workspace_bytes(self, steps: int, begin=True, end=False, window: int = None, head: int = None, tail: int = None) -> int:
        window, head, tail, flags = self._stream_args(window, head, tail, begin, end)
        return _lib.load().vit_hip_stream_workspace_bytes(self._handle._h, steps, window, head, tail, flags)

    def decode_stream(self, symbols, begin=True, end=False, window: int = None, head: int = None, tail: int = None, out=None,
                      workspace=None):
        """one segment [T][R] of ONE long unterminated stream, decoded as overlapped windows of `window` steps (default 1024) with
        `head` steps of lead-in and `tail` of look-ahead (default 8*(K-1) each): vit_hip_decode_stream.  begin: step 0 is the
        encoder's start (else the first `head` steps were emitted by the previous call); end: the last K-1 steps are the zero
        tail (else the last `tail` steps are look-ahead only: the next segment starts head + tail steps before this one's end).
        returns (bytes [ceil(n_bits/8)] uint8 on the device, MSB-first, pad bits 0; n_bits).  Segments of head + n*window + tail
        steps run as one uniform batch."""
        t = self.torch
        window, head, tail, flags = self._stream_args(window, head, tail, begin, end)
        if _args.dense(symbols, self._soft_dtype, None, "symbols").numel() % self.R != 0:
            raise ValueError("symbols must hold whole trellis steps, [steps][R]")
        T = symbols.numel() // self.R
        need = _lib.load().vit_hip_stream_workspace_bytes(self._handle._h, T, window, head, tail, flags)
        ws, nb = self._segment(need, workspace, T, head, tail, begin, end,
                               f"stream decoding needs head, tail >= K-1, window >= 8, head, tail, and a segment that emits bits "
                               f"(K = {self.K}, steps = {T}, window = {window}, head = {head}, tail = {tail})")
        out = t.empty(nb, dtype=t.uint8, device=self.device) if out is None else _args.dense(out, t.uint8, nb, "out")
        n_bits = C.c_size_t(0)
        _lib.check(_lib.load().vit_hip_decode_stream(
            self._handle._h, _ptr(symbols), T, window, head, tail, flags, _ptr(ws), ws.numel() * ws.element_size(), _ptr(out),
            C.byref(n_bits), self._stream()))
        return out, int(n_bits.value)

    def streams_workspace_bytes(self, n_streams: int, pitch: int, steps: int, begin=True, end=False, window: int = None,
                                head: int = None, tail: int = None) -> int:
        window, head, tail, flags = self._stream_args(window, head, tail, begin, end)
        return _lib.load().vit_hip_streams_workspace_bytes(self._handle._h, n_streams, pitch, steps, window, head, tail, flags)

    def decode_streams(self, symbols, steps: int = None, begin=True, end=False, window: int = None, head: int = None, tail: int = None,
                       out=None, workspace=None):
        """one segment of `steps` trellis steps of EACH of n_streams lockstep streams in one call: vit_hip_decode_streams.  symbols
        [n_streams][pitch][R], stream s in its first `steps` steps (default: all `pitch` of them), pitch a multiple of `window`; what
        lies behind `steps` is padding the result does not depend on.  begin / end / window / head / tail as decode_stream, shared
        by all streams.  returns (bytes [n_streams][ceil(n_bits/8)] uint8 on the device, n_bits): row s is what decode_stream returns
        for stream s.  `out`: a uint8 CUDA tensor [n_streams][>= ceil(n_bits/8)] with contiguous rows; the bytes of a row behind
        ceil(n_bits/8) are left as they are and the view of the written part is returned."""
        t = self.torch
        window, head, tail, flags = self._stream_args(window, head, tail, begin, end)
        if _args.dense(symbols, self._soft_dtype, None, "symbols").dim() != 3 or symbols.shape[2] != self.R:
            raise ValueError("symbols must be [n_streams][pitch][R]")
        n_streams, pitch = int(symbols.shape[0]), int(symbols.shape[1])
        T = pitch if steps is None else int(steps)
        need = _lib.load().vit_hip_streams_workspace_bytes(self._handle._h, n_streams, pitch, T, window, head, tail, flags)
        ws, nb = self._segment(need, workspace, T, head, tail, begin, end,
                               f"decoding lockstep streams needs what decode_stream needs, n_streams >= 1, pitch >= steps and pitch a "
                               f"multiple of the window (K = {self.K}, n_streams = {n_streams}, pitch = {pitch}, steps = {T}, "
                               f"window = {window}, head = {head}, tail = {tail})")
        if out is None:
            out = t.empty((n_streams, nb), dtype=t.uint8, device=self.device)
        elif (_args.device(out, t.uint8, "out").dim() != 2 or out.shape[0] != n_streams or out.shape[1] < nb or out.stride(1) != 1
              or (n_streams > 1 and out.stride(0) < nb)):
            raise ValueError(f"out must be [{n_streams}][>= {nb}] with contiguous rows")
        n_bits = C.c_size_t(0)
        _lib.check(_lib.load().vit_hip_decode_streams(
            self._handle._h, _ptr(symbols), n_streams, pitch, T, window, head, tail, flags, _ptr(ws), ws.numel() * ws.element_size(),
            _ptr(out), out.stride(0) if n_streams > 1 else nb, C.byref(n_bits), self._stream()))
        return out[:, :nb], int(n_bits.value)

    def depuncture(self, punctured, mask, out=None):
        """Depuncturing front-end (examples/helpers/puncture_code_helpers.h:17-55) for a batch: `punctured` is the device
        tensor [F][P] of transmitted symbols, `mask` the puncturing vector over one whole frame (truthy = transmitted, one
        entry per mother-code symbol, S*R in all); returns [F][S][R] with 0 (erasure) at the punctured positions.
        The map handed to vit_hip_depuncture_batch is the mask's exclusive prefix sum where the mask is set, -1 elsewhere.  The
        call's own rule is wider: entry j selects punctured[f][j] only where 0 <= j < P, every other entry -- negative, or at or
        above P -- reads as the erasure 0; whatever the map holds, nothing outside the buffers is read or written.  The call
        rejects (ValueError, nothing launched) buffers not aligned to the symbol type, a map not aligned to 4 bytes and an
        `out` that overlaps `punctured` or the map."""
        t = self.torch
        mask = np.asarray(mask).astype(bool).reshape(-1)
        if mask.size % self.R != 0:
            raise ValueError("the puncturing vector must cover whole trellis steps (a multiple of R symbols)")
        if _args.dense(punctured, self._soft_dtype, None, "punctured").dim() != 2 or punctured.shape[1] != int(mask.sum()):
            raise ValueError("punctured must be [frames][P] with the P symbols this puncturing vector keeps")
        d_idx = _args.puncture_map(self, mask)
        frames = punctured.shape[0]
        if out is None:
            out = t.empty((frames, mask.size // self.R, self.R), dtype=self._soft_dtype, device=self.device)
        _lib.check(_lib.load().vit_hip_depuncture_batch(self._handle._h, _ptr(punctured), punctured.shape[1], _ptr(d_idx), mask.size,
                                                        frames, _ptr(out), self._stream()))
        return out

    def lte_rate_dematch(self, received, D: int, E: int = None, offsets=None, counts=None, scramble=None, scramble_period: int = 0,
                         shift: int = 0, clamp=None, out=None):
        """LTE rate de-matching in front of decode_tail_biting (vit_hip_lte_rate_dematch_batch; 3GPP TS 36.212 5.1.4.2 undone): the
        demodulator's soft bits -> symbols [F][D][3], the repetitions of a coded bit added in int32, rounded by `shift` ((x + ((1 <<
        shift) >> 1)) >> shift) and clamped to `clamp` = (low, high), default the decoder's soft_decision_low / high; 0 where nothing
        was sent.  received: [F][>= E] of the decoder's symbol dtype, frame f in row f (E defaults to the row length), or with
        `offsets` (int32 CUDA [F]: element offsets, odd and overlapping ones included) one contiguous region of which nothing behind
        its end is read.  counts: int32 CUDA [F], the elements of each frame (cut at E), or None: E.  scramble: uint8 CUDA, the mask
        packed MSB-first (lte.lte_gold_sequence); the bit of region element g is g mod scramble_period (0: g) -- frames in rows of E
        with scramble_period=E share one mask.  The rule on the host: lte.lte_rate_dematch_numpy.  A decoder of rate 1/3 only.
        Nothing is copied to the host."""
        t = self.torch
        D, shift, period = int(D), int(shift), int(scramble_period)
        n, frames, stride, E = _args.lte_frames(received, self._soft_dtype, D, E, offsets, counts)
        if self.R != 3:
            raise ValueError("LTE rate de-matching feeds a rate 1/3 decoder")
        i = self._handle.info
        lo, hi = (i.soft_decision_low, i.soft_decision_high) if clamp is None else (int(clamp[0]), int(clamp[1]))
        if not 0 <= shift <= 15 or lo > hi or period < 0:
            raise ValueError("shift must be 0 .. 15, clamp = (low, high) with low <= high, scramble_period not negative")
        if scramble is not None and _args.dense(scramble, t.uint8, None, "scramble").numel() * 8 < (period or n):
            raise ValueError(f"scramble must hold {period or n} bits")
        if out is None:
            out = self._empty((frames, D, 3), self._soft_dtype)
        _args.dense(out, self._soft_dtype, frames * D * 3, "out")
        if frames == 0:
            return out
        _lib.check(_lib.load().vit_hip_lte_rate_dematch_batch(
            self._handle._h, _ptr(received), n, stride, _ptr(offsets), _ptr(counts), frames, D, E, _ptr(scramble), period, shift, lo, hi,
            _ptr(out), self._stream()))
        return out

    def wifi_deinterleave(self, soft, max_sym: int, S: int, rate: int = 0, rates=None, n_sym=None, n_steps=None, signal=None, out=None):
        """the 802.11a/g de-interleaver fused with depuncturing, in front of decode (vit_hip_wifi_deinterleave_batch): soft, a CUDA tensor
        of the decoder's symbol dtype [frames][>= max_sym * N_CBPS] with contiguous rows (frame f's OFDM symbols in transmit order; 288 a
        symbol where the rate is per frame) -> symbols [frames][S][2], which decode reads with L = S - 6.  rate: one index 0 .. 7 for all
        frames; or per frame on the device: rates / n_sym / n_steps, int32 CUDA [frames] each (None: `rate`, max_sym, n_sym * N_DBPS), or
        signal, the [frames][5] tensor wifi_signal_parse returned, whose rate_index, n_sym and n_steps columns are read in place.  Steps
        at or behind a frame's n_steps, punctured bits and frames of a rate above 7 are 0, the erasure.  The rule on the host:
        wifi.wifi_deinterleave_numpy.  A decoder of rate 1/2 only.  Nothing is copied to the host."""
        max_sym, S, rate = int(max_sym), int(S), int(rate)
        if self.R != 2:
            raise ValueError("the 802.11a/g data path feeds a rate 1/2 decoder")
        frames, stride = _args.wifi_soft(soft, self._soft_dtype, max_sym, S, rate, signal is not None or rates is not None)
        if signal is not None:
            if rates is not None or n_sym is not None or n_steps is not None:
                raise ValueError("signal stands for rates, n_sym and n_steps")
            at = _args.wifi_signal(signal, frames).data_ptr()
            p_rate, p_sym, p_steps, cs = C.c_void_p(at), C.c_void_p(at + 8), C.c_void_p(at + 12), 5
        else:
            for x, what in ((rates, "rates"), (n_sym, "n_sym"), (n_steps, "n_steps")):
                _args.counts(x, frames, what)
            p_rate, p_sym, p_steps, cs = _ptr(rates), _ptr(n_sym), _ptr(n_steps), 1
        if out is None:
            out = self._empty((frames, S, 2), self._soft_dtype)
        _args.dense(out, self._soft_dtype, frames * S * 2, "out")
        if frames == 0:
            return out
        _lib.check(_lib.load().vit_hip_wifi_deinterleave_batch(self._handle._h, _ptr(soft), stride, frames, max_sym, rate, p_rate, p_sym,
                                                               p_steps, cs, S, _ptr(out), self._stream()))
        return out

    def wifi_signal_parse(self, bytes, out=None):
        """the 802.11a/g SIGNAL field (vit_hip_wifi_signal_batch): bytes, uint8 CUDA [frames][>= 3] with contiguous rows -- what decode
        returns with L = 18 for the SIGNAL symbol de-interleaved at rate 0, max_sym 1, S 24 -- -> int32 CUDA [frames][5] = (rate_index,
        length, n_sym, n_steps, valid), the uint32 values of the ABI: rate_index 8 for an unknown pattern; valid = 1 where the pattern
        is known, the parity holds, the reserved bit is 0 and length >= 1; n_steps = 16 + 8 length + 6 and n_sym = ceil(n_steps / N_DBPS)
        where valid, else 0.  The rule on the host: wifi.wifi_signal_parse_numpy.  Nothing is copied to the host."""
        t = self.torch
        frames, stride = _args.wifi_rows(bytes, t.uint8, 3, "bytes")
        if out is None:
            out = self._empty((frames, 5), t.int32)
        _args.wifi_signal(out, frames, "out")
        if frames == 0:
            return out
        _lib.check(_lib.load().vit_hip_wifi_signal_batch(self._handle._h, _ptr(bytes), stride, frames, _ptr(out), self._stream()))
        return out

    def wifi_descramble(self, bytes, S: int, lengths, max_length: int = None, out=None):
        """descrambling, PSDU octets and the FCS of 802.11a/g DATA fields (vit_hip_wifi_data_batch): bytes, uint8 CUDA [frames][>=
        ceil((S - 6) / 8)] with contiguous rows, what decode returns with L = S - 6.  lengths: int32 CUDA [frames], or the [frames][5]
        tensor wifi_signal_parse returned, whose length column is read in place.  A frame's length is cut at max_length (None: what S
        holds, (S - 22) / 8) and at what S holds.  returns (psdu, status): uint8 [frames][max_length] of which frame f's first
        length_used octets are written, and int32 [frames][4] = (length_used, seed, service, fcs_syndrome), the uint32 values of the
        ABI: seed the scrambler's first seven bits (0: not a scrambler's), service 0 from a conforming sender, fcs_syndrome =
        zlib.crc32(psdu[:-4]) ^ the last four octets read little-endian: 0 where the frame checks, 0xFFFFFFFF below four octets.  out =
        (psdu, status) reuses those tensors; psdu rows may be wider.  The rule on the host: wifi.wifi_descramble_numpy.  Nothing is
        copied to the host."""
        t = self.torch
        S = int(S)
        if S < 22:
            raise ValueError("S must be at least 22: the SERVICE field and the tail")
        room = (S - 22) // 8
        max_length = room if max_length is None else int(max_length)
        if max_length < 0:
            raise ValueError("max_length must not be negative")
        frames, stride = _args.wifi_rows(bytes, t.uint8, (S - 6 + 7) // 8, "bytes")
        if lengths.dim() == 2:
            at, ls = C.c_void_p(_args.wifi_signal(lengths, frames, "lengths").data_ptr() + 4), 5
        else:
            at, ls = _ptr(_args.dense(lengths, t.int32, frames, "lengths")), 1
        if out is None:
            out = (self._empty((frames, max_length), t.uint8), self._empty((frames, 4), t.int32))
        psdu, status = out
        pframes, pstride = _args.wifi_rows(psdu, t.uint8, min(max_length, room), "out[0]")
        if pframes != frames or psdu.dim() != 2:
            raise ValueError(f"out[0] must hold [{frames}] rows")
        _args.dense(status, t.int32, frames * 4, "out[1]")
        if frames == 0:
            return psdu, status
        at_psdu = _ptr(psdu) if psdu.numel() else C.c_void_p(status.data_ptr())        # no octet is written: any non-NULL address
        _lib.check(_lib.load().vit_hip_wifi_data_batch(self._handle._h, _ptr(bytes), stride, frames, S, at, ls, max_length, at_psdu,
                                                       pstride, _ptr(status), self._stream()))
        return psdu, status

    def dvbt_deinterleave(self, symbols, mode, v: int, rate: int, parity=0, out=None):
        """the DVB-T inner de-interleaver (symbol, bit, demultiplexer) fused with depuncturing, in front of decode_stream(s)
        (vit_hip_dvbt_deinterleave_batch; ETSI EN 300 744 clauses 4.3.3, 4.3.4).  symbols: a CUDA tensor of the decoder's symbol dtype
        [rows][n_sym][Nmax * v] (or [n_sym][Nmax * v]: one row), every OFDM symbol's data cells in carrier order, v soft bits a cell; a
        view with a larger row stride is read in place.  mode '2k', '4k' or '8k'; v 2, 4 or 6; rate 0 .. 4 = 1/2, 2/3, 3/4, 5/6, 7/8.
        parity: that of every row's first symbol, an int -- or (counter_in, counter_out), two distinct int32 CUDA tensors [rows]: the
        first holds every row's parity (any count: its lowest bit), the second receives it plus n_sym, and the next call takes them the
        other way round.  returns [rows][n_sym * steps][2] ([n_sym * steps][2] for one row given as such), (Y, X) per trellis step, 0
        where the rate sent nothing; out = a tensor [rows][>= n_sym * steps][2] with contiguous rows is written in place, nothing behind
        a row's steps touched.  The rule on the host: dvbt.dvbt_deinterleave_numpy.  A decoder of rate 1/2 only.  Nothing is copied to
        the host."""
        from . import dvbt
        t = self.torch
        m = dvbt._mode(mode)
        v, rate = dvbt._check(v, rate)
        if self.R != 2:
            raise ValueError("the DVB-T front end feeds a rate 1/2 decoder")
        rows, n_sym, stride = _args.dvbt_symbols(symbols, self._soft_dtype, m.n_max * v)
        steps = n_sym * dvbt.dvbt_steps_per_symbol(m, v, rate)
        first, p_in, p_out = 0, None, None
        if isinstance(parity, (tuple, list)):
            p_in, p_out = parity
            _args.dense(p_in, t.int32, rows, "parity[0]"), _args.dense(p_out, t.int32, rows, "parity[1]")
            if p_in.data_ptr() == p_out.data_ptr():
                raise ValueError("the two parity counters must be distinct tensors")
        else:
            first = int(parity) & 1
        if out is None:
            out = self._empty((rows, steps, 2) if symbols.dim() == 3 else (steps, 2), self._soft_dtype)
        pitch = _args.dvbt_out(out, self._soft_dtype, rows, steps)
        if rows == 0 or n_sym == 0:
            return out
        _lib.check(_lib.load().vit_hip_dvbt_deinterleave_batch(self._handle._h, _ptr(symbols), stride, rows, n_sym, m.index, v, rate, first,
                                                               _ptr(p_in), _ptr(p_out), _ptr(out), pitch, self._stream()))
        return out

    def is95_deinterleave(self, symbols, scramble=None, shift: int = 0, clamp=None, out=None, want=(True, True, True, True)):
        """the IS-95A forward traffic channel in front of decode (vit_hip_is95_deinterleave_batch): long-code descrambling, the 384-symbol
        block de-interleaver and the combining of the repetitions under the four rate hypotheses, in one launch.  symbols: a CUDA tensor
        of the decoder's symbol dtype [frames][>= 384] with contiguous rows (or one frame), a view with a larger row stride read in
        place; scramble: uint8 CUDA, the mask packed MSB-first, [48] for the whole batch or [frames][>= 48] with contiguous rows, None:
        off.  The repetitions are added in int32, rounded by `shift` ((x + ((1 << shift) >> 1)) >> shift) and clamped to `clamp` = (low,
        high), default the decoder's soft_decision_low / high.  returns four tensors [frames][S_h][2], S_h = 192, 96, 48, 24, which
        decode reads with L = 184, 88, 40, 16; `want` leaves hypotheses out (None in their place), out = four such tensors (None: not
        wanted) are written in place; they must not share storage.  The rule on the host: is95.is95_deinterleave_numpy.  A decoder of
        rate 1/2 only.  Nothing is copied to the host."""
        from .is95 import IS95_RATE_SET_1
        shift = int(shift)
        if self.R != 2:
            raise ValueError("the IS-95 traffic channel feeds a rate 1/2 decoder")
        i = self._handle.info
        lo, hi = (i.soft_decision_low, i.soft_decision_high) if clamp is None else (int(clamp[0]), int(clamp[1]))
        if not 0 <= shift <= 15 or lo > hi:
            raise ValueError("shift must be 0 .. 15, clamp = (low, high) with low <= high")
        frames, stride, sstride = _args.is95_symbols(symbols, self._soft_dtype, scramble)
        if out is None:
            out = tuple(self._empty((frames, r.steps, 2), self._soft_dtype) if w else None for r, w in zip(IS95_RATE_SET_1, want))
        out = _args.is95_outputs(out, self._soft_dtype, frames)
        if frames == 0:
            return out
        at = (C.c_void_p * 4)(*[None if x is None else x.data_ptr() for x in out])
        _lib.check(_lib.load().vit_hip_is95_deinterleave_batch(self._handle._h, _ptr(symbols), stride, frames, _ptr(scramble), sstride, shift,
                                                               lo, hi, at, self._stream()))
        return out

    def is95_channel_errors(self, symbols, bytes, out=None):
        """the re-encoded symbol error counts of the four IS-95A hypotheses in one call (vit_hip_is95_channel_errors_batch): symbols, the
        four tensors is95_deinterleave returned, and bytes, what decode returned for them (uint8 [frames][>= 23 / 11 / 5 / 2] with
        contiguous rows; None: a hypothesis left out).  returns (errors, compared), two lists of four int32 CUDA tensors [frames] (None
        where left out) that hold what channel_errors(symbols[h], bytes[h], L_h) returns; out = (errors, compared) reuses such lists.
        The counters are zeroed by a kernel, not by memsets, so a captured graph holds no memset node.  A K = 9, R = 1/2 decoder only.
        Nothing is copied to the host."""
        t = self.torch
        if (self.K, self.R) != (9, 2):
            raise ValueError("the IS-95 traffic channel needs a K = 9, R = 1/2 decoder")
        frames, strides = _args.is95_decoded(bytes, None, None, None)
        if out is None:
            out = tuple([None if b is None else self._empty((frames,), t.int32) for b in bytes] for _ in range(2))
        errors, compared = out
        _args.is95_counted(symbols, bytes, errors, compared, self._soft_dtype, frames)
        if frames == 0:
            return errors, compared
        ptrs = lambda xs: (C.c_void_p * 4)(*[None if x is None or bytes[k] is None else x.data_ptr() for k, x in enumerate(xs)])
        _lib.check(_lib.load().vit_hip_is95_channel_errors_batch(self._handle._h, ptrs(symbols), ptrs(bytes), (C.c_size_t * 4)(*strides), frames,
                                                                 ptrs(errors), ptrs(compared), self._stream()))
        return errors, compared

    def is95_rate_decide(self, bytes, errors, compared, syndrome, max_ser_num, ser_den: int, out=None):
        """the blind rate decision of the IS-95A forward traffic channel and the winner's info bits (vit_hip_is95_rate_decide_batch).
        bytes: four uint8 CUDA tensors [frames][>= 23 / 11 / 5 / 2] with contiguous rows, what decode returned for the four outputs of
        is95_deinterleave, None for a hypothesis out of the contest; errors, compared: four int32 CUDA tensors [frames] each, what
        channel_errors returned (not read for an absent hypothesis, which may give None); syndrome: two, what crc_check returned with
        is95.IS95_CRC12 over 172 bits and IS95_CRC8 over 80.  Hypothesis h passes with a zero syndrome (h < 2), compared > 0 and errors *
        ser_den <= compared * max_ser_num[h]; the passing one with the lowest errors / compared wins, the lower h on a tie.  returns
        (decision int32 [frames][4] = (rate, info_bits, errors, compared), the uint32 values of the ABI, rate 4 and zeros for an erased
        frame; info uint8 [frames][22], the winner's info bits, zero behind them); out = (decision, info) reuses those tensors, info
        rows may be wider.  The rule on the host: is95.is95_rate_decide_numpy.  Nothing is copied to the host."""
        from .is95 import IS95_INFO_BYTES, IS95_RATE_SET_1
        t = self.torch
        frames, strides = _args.is95_decoded(bytes, errors, compared, syndrome)
        num = [int(n) for n in max_ser_num]
        if len(num) != 4 or int(ser_den) < 1 or min(num) < 0 or max(num + [int(ser_den)]) > 0xFFFFFFFF:
            raise ValueError("max_ser_num must be four uint32 values, ser_den 1 .. 2^32 - 1")
        if out is None:
            out = (self._empty((frames, 4), t.int32), self._empty((frames, IS95_INFO_BYTES), t.uint8))
        decision, info = out
        _args.dense(decision, t.int32, frames * 4, "out[0]")
        iframes, istride = _args.wifi_rows(info, t.uint8, IS95_INFO_BYTES, "out[1]")
        if iframes != frames or info.dim() != 2:
            raise ValueError(f"out[1] must hold [{frames}] rows")
        if frames == 0:
            return decision, info
        ptrs = lambda xs, n: (C.c_void_p * n)(*[None if x is None or bytes[k] is None else x.data_ptr() for k, x in enumerate(xs[:n])])
        _lib.check(_lib.load().vit_hip_is95_rate_decide_batch(
            self._handle._h, ptrs(bytes, 4), (C.c_size_t * 4)(*strides), ptrs(errors, 4), ptrs(compared, 4), ptrs(syndrome, 2), frames,
            (C.c_uint32 * 4)(*num), int(ser_den), _ptr(decision), _ptr(info), istride, self._stream()))
        return decision, info

    def gsm_deinterleave(self, bursts, mode, negate: bool = False, hist=None, fill=None, out=None,
                         want=("full", "class1", "class2", "steal")):
        """the GSM burst de-interleaver in front of decode (vit_hip_gsm_deinterleave_batch; 3GPP TS 45.003).  bursts: a CUDA tensor of the
        decoder's symbol dtype [rows][4 m][>= 116] (or [4 m][...]: one row), e(B, 0 .. 115) with the stealing flags at 57 and 58; a view
        with larger strides is read in place.  mode gsm.GSM_BLOCK (control channels: 4 bursts a block, no history) or gsm.GSM_DIAGONAL
        (TCH/F, FACCH/F: 8 bursts a block with half-block overlap; hist / fill: the hist_out [rows][464] and fill_out int32 [rows] the
        call before returned, None: no history, and a row gives m - 1 blocks).  negate: every value negated on the way, clamped to the
        dtype.  returns a dict: full [rows][m][228][2] (decode reads it with L = 224), class1 [rows][m][189][2] (L = 185), class2
        [rows][m][78], steal int32 [rows][m] (the sum of the block's stealing flags), n_out int32 [rows] (the blocks the row gave; the
        slots behind them are zeros) and, in diagonal mode, hist_out, fill_out; `want` names which of the first four are allocated, out
        = a dict of such tensors is written in place and nothing else.  The rule on the host: gsm.gsm_deinterleave_numpy.  A decoder of
        rate 1/2 only.  Nothing is copied to the host."""
        from . import gsm
        t = self.torch
        mode = gsm._mode(mode)
        if self.R != 2:
            raise ValueError("the GSM burst de-interleaver feeds a rate 1/2 decoder")
        rows, n_bursts, rs, bs = _args.gsm_bursts(bursts, self._soft_dtype)
        m = n_bursts // 4
        if mode == gsm.GSM_BLOCK and (hist is not None or fill is not None):
            raise ValueError("the block mode carries no history")
        if (hist is None) != (fill is None):
            raise ValueError("hist and fill come together")
        if hist is not None:
            _args.dense(hist, self._soft_dtype, rows * 464, "hist"), _args.dense(fill, t.int32, rows, "fill")
        if out is None:
            shapes = {"full": (rows, m, 228, 2), "class1": (rows, m, 189, 2), "class2": (rows, m, 78)}
            out = {k: self._empty((rows, m), t.int32) if k == "steal" else self._empty(shapes[k], self._soft_dtype) for k in want}
            out["n_out"] = self._empty((rows,), t.int32)
            if mode == gsm.GSM_DIAGONAL:
                out["hist_out"], out["fill_out"] = self._empty((rows, 464), self._soft_dtype), self._empty((rows,), t.int32)
        got = _args.gsm_outputs(out, self._soft_dtype, rows, m, mode == gsm.GSM_DIAGONAL)
        result = dict(zip(("hist_out", "fill_out", "n_out", "full", "class1", "class2", "steal"), got))
        if rows == 0 or m == 0:
            return result
        _lib.check(_lib.load().vit_hip_gsm_deinterleave_batch(self._handle._h, _ptr(bursts), rs, bs, rows, n_bursts, mode,
                                                              _lib.GSM_NEGATE if negate else 0, _ptr(hist), _ptr(fill), *[_ptr(x) for x in got],
                                                              self._stream()))
        return result

    def gsm_fire(self, bytes, max_burst: int = 12, lsb_first: bool = False, out=None):
        """the Fire code of the GSM control channels (vit_hip_gsm_fire_batch): bytes, uint8 CUDA [frames][>= 28] with contiguous rows, what
        decode returns with L = 224 -- 184 data bits, 40 parity bits.  A frame whose syndrome is not 0 is searched for the one error burst
        of at most max_burst (0 .. 12; 0: detect only) bits that explains it, and that burst is flipped.  returns (status int32 [frames][4]
        = (status, first_bit, syndrome_lo, syndrome_hi): status 0 clean, 1 .. 12 the length of the corrected burst from bit first_bit on,
        -1 not correctable; data uint8 [frames][23], MSB-first or, with lsb_first, d(8 i + b) as bit b of byte i).  out = (status, data)
        reuses those tensors; data rows may be wider, and data may be `bytes` itself: in place.  The rule on the host:
        gsm.gsm_fire_numpy.  Nothing is copied to the host."""
        t = self.torch
        max_burst = int(max_burst)
        if not 0 <= max_burst <= 12:
            raise ValueError("max_burst must be 0 .. 12")
        frames, stride = _args.wifi_rows(bytes, t.uint8, 28, "bytes")
        if out is None:
            out = (self._empty((frames, 4), t.int32), self._empty((frames, 23), t.uint8))
        status, data = out
        _args.dense(status, t.int32, frames * 4, "out[0]")
        dframes, dstride = _args.wifi_rows(data, t.uint8, 23, "out[1]")
        if dframes != frames:
            raise ValueError(f"out[1] must hold [{frames}] rows")
        if data.data_ptr() == bytes.data_ptr() and frames == 1:
            dstride = stride
        if frames == 0:
            return status, data
        _lib.check(_lib.load().vit_hip_gsm_fire_batch(self._handle._h, _ptr(bytes), stride, frames, max_burst,
                                                      _lib.GSM_LSB_FIRST if lsb_first else 0, _ptr(status), _ptr(data), dstride, self._stream()))
        return status, data

    def gsm_tchfs(self, bytes, class2, out=None):
        """the GSM TCH/FS frame behind decode (vit_hip_gsm_tchfs_batch): bytes, uint8 CUDA [frames][>= 24] with contiguous rows, what decode
        returns with L = 185 for the class1 output of gsm_deinterleave, and class2, its class2 output as [frames][78].  returns (speech
        uint8 [frames][33]: the 260 bits MSB-first -- class I reordered, class II by hard decision against the decoder's
        soft_decision_high / low --, the last four bits 0; status int32 [frames][2] = (parity_syndrome: 0 where the 3 parity bits over the
        first 50 bits hold, class2_erasures: class II values at the midpoint)).  out = (speech, status) reuses those tensors; speech rows
        may be wider.  The rule on the host: gsm.gsm_tchfs_numpy.  Nothing is copied to the host."""
        t = self.torch
        frames, stride = _args.wifi_rows(bytes, t.uint8, 24, "bytes")
        _args.dense(class2, self._soft_dtype, frames * 78, "class2")
        if out is None:
            out = (self._empty((frames, 33), t.uint8), self._empty((frames, 2), t.int32))
        speech, status = out
        sframes, sstride = _args.wifi_rows(speech, t.uint8, 33, "out[0]")
        if sframes != frames:
            raise ValueError(f"out[0] must hold [{frames}] rows")
        _args.dense(status, t.int32, frames * 2, "out[1]")
        if frames == 0:
            return speech, status
        _lib.check(_lib.load().vit_hip_gsm_tchfs_batch(self._handle._h, _ptr(bytes), stride, _ptr(class2), frames, _ptr(speech), sstride,
                                                       _ptr(status), self._stream()))
        return speech, status

    def dab_deinterleave(self, frames, n_frames=None, source_index=None, hist=None, fill=None, n_received: int = None, out=None):
        """the DAB time de-interleaver fused with depuncturing, in front of decode (vit_hip_dab_deinterleave_batch; ETSI EN 300 401
        clauses 12 and 11).  frames: the received soft bits, a CUDA tensor of the decoder's symbol dtype [rows][max_frames][>= n] (or
        [max_frames][...]: one row; n = n_received, by default the last dimension) -- a view with larger strides, a sub-channel cut out
        of whole CIFs, is read in place.  n_frames: int32 CUDA [rows] or None: all.  source_index: int32 CUDA [symbols_per_frame], the
        received soft bit every output symbol is (dab.DabProfile.source_index(); an entry outside 0 .. n-1 gives 0, the erasure), or
        None: the identity, the de-interleaver alone.  hist / fill: the [rows][15 n] and int32 [rows] the previous call returned as
        hist_out / fill_out (None: nothing carried).  returns (out, n_out, hist_out, fill_out): [rows][max_frames][symbols_per_frame]
        of which the first n_out[r] (int32 [rows]) frames of row r are written -- symbol q of frame k is soft bit p = source_index[q] of
        frame k + bitrev4(p mod 16) of the real history frames followed by the input --, and the last min(15, all) frames of that
        sequence with their number.  out = the same four reuses those tensors; hist and hist_out must be distinct and have the same row
        stride.  The rule on the host: dab.dab_time_deinterleave_numpy and dab.dab_depuncture_numpy.  Nothing is copied to the host."""
        t = self.torch
        n = int(frames.shape[-1]) if n_received is None else int(n_received)
        if n < 1:
            raise ValueError("n_received must be at least 1")
        rows, mf, rs, fs = _args.soft_frames(frames, self._soft_dtype, "frames", n)
        if rows == 0 or mf == 0:
            raise ValueError("frames holds no frame: a call without input changes nothing")
        spf = n if source_index is None else _args.dense(source_index, t.int32, None, "source_index").numel()
        if spf < 1:
            raise ValueError("source_index must hold at least one entry")
        if out is None:
            out = (self._empty((rows, mf, spf), self._soft_dtype), self._empty(rows, t.int32), self._empty((rows, 15 * n), self._soft_dtype),
                   self._empty(rows, t.int32))
        d_out, n_out, hist_out, fill_out = out
        _args.dense(d_out, self._soft_dtype, rows * mf * spf, "out[0]")
        _args.counts(n_frames, rows, "n_frames"), _args.dense(n_out, t.int32, rows, "out[1]"), _args.dense(fill_out, t.int32, rows, "out[3]")
        hstride = _args.carried(hist, fill, hist_out, rows, 15 * n, "hist", "fill", self._soft_dtype)
        _lib.check(_lib.load().vit_hip_dab_deinterleave_batch(
            self._handle._h, _ptr(frames), rs, fs, rows, mf, _ptr(n_frames), n, _ptr(source_index), spf, _ptr(hist),
            _ptr(fill) if hist is not None else None, hstride, _ptr(d_out), _ptr(n_out), _ptr(hist_out), _ptr(fill_out), self._stream()))
        return d_out, n_out, hist_out, fill_out

    def synth(self, frames: int, L: int, ebn0_db, seed: int = 1, first_frame: int = 0, tx_out=None, symbols_out=None):
        """synthetic AWGN frames of this decoder's code, generated in HBM by one HIP kernel (vit_hip_synth_batch: the
        reference BER harness's generator, examples/run_snr_ber.cpp:311-359).  ebn0_db=None: noise-free symbols at exactly
        high / low.  returns (tx_bytes [F][L/8] uint8, symbols [F][L+K-1][R] soft dtype), both on the device."""
        t = self.torch
        tx = t.empty((frames, L // 8), dtype=t.uint8, device=self.device) if tx_out is None else tx_out
        sym = t.empty((frames, L + self.K - 1, self.R), dtype=self._soft_dtype, device=self.device) if symbols_out is None else symbols_out
        _lib.check(_lib.load().vit_hip_synth_batch(self._handle._h, frames, L, int(seed), int(first_frame),
                                                   0.0 if ebn0_db is None else float(ebn0_db), 1 if ebn0_db is None else 0,
                                                   _ptr(tx), _ptr(sym), self._stream()))
        return tx, sym

    def count_bit_errors(self, a, b, count=None):
        """number of differing bits between two device byte tensors (get_total_bit_errors, test_helpers.h:95-104), added to
        the one-element int64 device tensor `count` (created zeroed when None); no host synchronisation."""
        t = self.torch
        if a.dtype != t.uint8 or b.dtype != t.uint8 or a.numel() != b.numel() or not (a.is_contiguous() and b.is_contiguous()):
            raise ValueError("need two contiguous uint8 tensors of equal size")
        if count is None:
            count = t.zeros(1, dtype=t.int64, device=self.device)
        _lib.check(_lib.load().vit_hip_count_bit_errors(self._handle._h, _ptr(a), _ptr(b), a.numel(), _ptr(count), self._stream()))
        return count

    def _encode_args(self, bytes, L, tail, tail_biting, start_state, bytes_frame_stride=0):
        """(frames, flags, steps, byte stride, start-state tensor or None) of an encode / channel_errors call"""
        t = self.torch
        if tail_biting and start_state is not None:
            raise ValueError("a tail-biting frame takes its start state from its own last K-1 bits")
        flags = _lib.ENCODE_TAIL_BITING if tail_biting else (_lib.ENCODE_TAIL if tail else 0)
        steps = L + (self.K - 1 if flags == _lib.ENCODE_TAIL else 0)
        nb = (L + 7) // 8
        if _args.device(bytes, t.uint8, "bytes").dim() not in (1, 2) or bytes.stride(-1) != 1:
            raise ValueError("bytes must be [frames][>= ceil(L/8)] (or one frame's bytes) with contiguous rows")
        if bytes.dim() == 2:
            frames = int(bytes.shape[0])
            stride = int(bytes_frame_stride) or (int(bytes.stride(0)) if frames > 1 else int(bytes.shape[1]))
            if bytes.shape[1] < nb:
                raise ValueError(f"{L} bits need {nb} bytes per frame")
        else:
            stride = int(bytes_frame_stride) or nb
            frames = (bytes.numel() - nb) // stride + 1 if bytes.numel() >= nb else 0
        if frames < 1 or stride < nb:
            raise ValueError(f"bytes holds no frame of {nb} bytes at stride {stride}")
        return frames, flags, steps, stride, _args.state_tensor(t, self.device, start_state, frames)

    def encode(self, bytes, L: int, tail=True, tail_biting=False, start_state=None, out=None, end_state_out=False):
        """the convolutional encoder on device-resident info bytes (vit_hip_encode_batch): bytes [F][>= ceil(L/8)] uint8, MSB-first
        as chainback() writes them -> symbols [F][steps][R] at exactly soft_decision_high / low, steps = L + K-1 with `tail`
        (K-1 zero bits follow), L with tail=False (an unterminated piece of a stream, from `start_state` [F], None = 0) or with
        `tail_biting` (the frame starts in the state its last K-1 bits leave).  States are numbered as update()'s start_state
        and chainback()'s end_state.  `out`: a symbol tensor of steps*R elements per frame, or a 2-D one [F][>= steps*R] whose
        row stride is the frame stride (what lies behind steps*R is left as it is).  end_state_out: True (or an int32 tensor [F])
        returns (symbols, end_state): the state after each frame's last step."""
        t = self.torch
        frames, flags, steps, bstride, ss = self._encode_args(bytes, L, tail, tail_biting, start_state)
        n = steps * self.R
        if out is None:
            out = t.empty((frames, steps, self.R), dtype=self._soft_dtype, device=self.device)
        if _args.device(out, self._soft_dtype, "out").is_contiguous() and out.numel() == frames * n:
            sstride = n
        elif out.dim() == 2 and out.shape[0] == frames and out.shape[1] >= n and out.stride(1) == 1 and (frames == 1 or out.stride(0) >= n):
            sstride = int(out.stride(0)) if frames > 1 else n
        else:
            raise ValueError(f"out must hold {frames} x {n} symbols, or be [frames][>= {n}] with contiguous rows")
        es = None
        if end_state_out is not False and end_state_out is not None:
            es = t.empty(frames, dtype=t.int32, device=self.device) if end_state_out is True else end_state_out
            _args.dense(es, t.int32, frames, "end_state_out")
        _lib.check(_lib.load().vit_hip_encode_batch(
            self._handle._h, _ptr(bytes), bstride, frames, L, flags, _ptr(ss), _ptr(out), sstride, _ptr(es), self._stream()))
        return (out, es) if es is not None else out

    def channel_errors(self, symbols, bytes, L: int, tail=True, tail_biting=False, start_state=None, symbol_frame_stride: int = 0,
                       bytes_frame_stride: int = 0):
        """the re-encoded channel symbol error count (vit_hip_channel_errors_batch): the decoded `bytes` [F][>= ceil(L/8)] are
        encoded again in registers (tail / tail_biting / start_state as encode()) and compared with the hard decisions of the
        received `symbols`.  returns (errors, compared), int32 device tensors [F]: compared = symbols that are not at the
        midpoint (high + low)/2 -- erasures, such as the 0 depuncture() inserts, are skipped --, errors = compared symbols whose
        hard decision differs from the re-encoded bit.  errors / compared is the channel symbol error rate.
        symbols: frame f's [steps][R] start at element f * symbol_frame_stride of the tensor (0: the row stride of a [F][...]
        tensor, else packed); it may be a view into a larger buffer.  bytes_frame_stride likewise (0: the row stride)."""
        t = self.torch
        frames, flags, steps, bstride, ss = self._encode_args(bytes, L, tail, tail_biting, start_state, bytes_frame_stride)
        n = steps * self.R
        if _args.device(symbols, self._soft_dtype, "symbols").stride(-1) != 1:
            raise ValueError("the last dimension of symbols must be contiguous")
        sstride = int(symbol_frame_stride)
        if sstride == 0:
            if symbols.is_contiguous() and symbols.numel() == frames * n:
                sstride = n
            elif symbols.dim() >= 2 and symbols.shape[0] == frames and symbols[0].is_contiguous() and symbols[0].numel() >= n:
                sstride = int(symbols.stride(0)) if frames > 1 else n
            else:
                raise ValueError(f"symbols must hold {frames} x {n} symbols, or pass symbol_frame_stride")
        room = symbols.untyped_storage().nbytes() // symbols.element_size() - symbols.storage_offset()
        if sstride < n or room < (frames - 1) * sstride + n:
            raise ValueError(f"{frames} frames of {n} symbols at stride {sstride} do not fit the symbol tensor")
        err = t.empty(frames, dtype=t.int32, device=self.device)
        cmp = t.empty(frames, dtype=t.int32, device=self.device)
        _lib.check(_lib.load().vit_hip_channel_errors_batch(
            self._handle._h, _ptr(symbols), sstride, _ptr(bytes), bstride, frames, L, flags, _ptr(ss), _ptr(err), _ptr(cmp),
            self._stream()))
        return err, cmp

    def _sync_args(self, received, hypotheses, mask):
        """(hypothesis array, count, source map tensor or None, period_symbols, kept_per_period) of a sync_build / sync_search call"""
        t = self.torch
        if _args.dense(received, self._soft_dtype, None, "received").dim() != 1:
            raise ValueError("received must be 1-D")
        hyps = [(int(o), int(f)) for o, f in hypotheses]
        if not 1 <= len(hyps) <= _lib.SYNC_MAX_HYPOTHESES:
            raise ValueError(f"1 to {_lib.SYNC_MAX_HYPOTHESES} hypotheses per call")
        arr = (_lib.VitHipSyncHypothesis * len(hyps))(*hyps)
        if mask is None:
            return arr, len(hyps), None, 0, 0
        mask = np.asarray(mask).astype(bool).reshape(-1)
        if mask.size == 0 or mask.size % self.R != 0 or not mask.any():
            raise ValueError("the puncturing mask must cover whole trellis steps (a multiple of R symbols) and keep a symbol")
        return arr, len(hyps), _args.puncture_map(self, mask), mask.size, int(mask.sum())

    def sync_build(self, received, hypotheses, steps: int, mask=None, pitch: int = None, out=None):
        """the [steps][R] stream of every alignment hypothesis from ONE received buffer (vit_hip_sync_build): hypotheses is a
        sequence of (offset, flags) -- offset = received symbols in front of a puncturing period, flags of _lib.SYNC_SWAP_PAIRS /
        SYNC_NEGATE_EVEN / SYNC_NEGATE_ODD (sync.enumerate_hypotheses makes the usual sets) --, mask the 0/1 puncturing mask over ONE
        period as depuncture() takes it (None: unpunctured).  returns [n_hyp][pitch][R] (pitch in steps, default `steps`); the steps
        behind `steps` are not written.  One hypothesis with the default pitch is what decode_stream / StreamDecoder.push read."""
        t = self.torch
        arr, n, d_idx, period, kept = self._sync_args(received, hypotheses, mask)
        steps = int(steps)
        pitch = steps if pitch is None else int(pitch)
        if out is None:
            out = t.empty((n, pitch, self.R), dtype=self._soft_dtype, device=self.device)
        else:
            _args.dense(out, self._soft_dtype, n * pitch * self.R, "out")
        _lib.check(_lib.load().vit_hip_sync_build(self._handle._h, _ptr(received), received.numel(), _ptr(d_idx), period, kept, arr, n,
                                                  steps, pitch, _ptr(out), self._stream()))
        return out

    def sync_search_workspace_bytes(self, n_hyp: int, steps: int, window: int = None, head: int = None, tail: int = None) -> int:
        window, head, tail, _ = self._stream_args(window, head, tail, False, False)
        return _lib.load().vit_hip_sync_search_workspace_bytes(self._handle._h, int(n_hyp), int(steps), window, head, tail)

    def sync_search(self, received, hypotheses, steps: int, mask=None, window: int = None, head: int = None, tail: int = None,
                    workspace=None):
        """node synchronisation in one call (vit_hip_sync_search): the streams of all hypotheses (as sync_build) are decoded as
        mid-stream segments of `steps` steps (window / head / tail as decode_streams), re-encoded from the decoded bits and compared
        with their own symbols.  returns (errors, compared, best): int32 CUDA tensors [n_hyp], [n_hyp] and [1] -- the re-encoded
        channel symbol error count of every hypothesis and the index of the one with the lowest rate (the lower index on a tie:
        on a transparent code an inverted stream ties with the upright one).  Nothing is copied to the host."""
        t = self.torch
        arr, n, d_idx, period, kept = self._sync_args(received, hypotheses, mask)
        steps = int(steps)
        window, head, tail, _ = self._stream_args(window, head, tail, False, False)
        need = _lib.load().vit_hip_sync_search_workspace_bytes(self._handle._h, n, steps, window, head, tail)
        if need == 0:
            raise ValueError(f"a synchronisation search needs what decode_streams needs and more than 8*ceil((K-1)/8) emitted bits, on "
                             f"a linear code (K = {self.K}, steps = {steps}, window = {window}, head = {head}, tail = {tail})")
        ws = self._scratch(need, workspace)
        err = t.empty(n, dtype=t.int32, device=self.device)
        cmp = t.empty(n, dtype=t.int32, device=self.device)
        best = t.empty(1, dtype=t.int32, device=self.device)
        _lib.check(_lib.load().vit_hip_sync_search(
            self._handle._h, _ptr(received), received.numel(), _ptr(d_idx), period, kept, arr, n, steps, window, head, tail, _ptr(ws),
            ws.numel() * ws.element_size(), _ptr(err), _ptr(cmp), _ptr(best), self._stream()))
        return err, cmp, best

    def export_decisions(self, frames: int, L: int, n_steps: int = None, workspace=None, first_frame: int = 0):
        """decision history in the reference layout: int64 tensor [F][n_steps][W] (bit pattern of uint64 words).  The
        workspace is an array of independent slabs of `workspace_tile_frames` frames (vit_hip_info), so `frames` frames
        starting at a slab-aligned `first_frame` of a larger batch can be exported on their own."""
        t = self.torch
        n_steps = (L + self.K - 1) if n_steps is None else n_steps
        if first_frame:
            self._handle.refresh()
            tile = self._handle.info.workspace_tile_frames
            if first_frame % tile:
                raise ValueError(f"first_frame must be a multiple of {tile} for this plan")
            base = self._ws if workspace is None else workspace
            workspace = base[(first_frame // tile) * _lib.load().vit_hip_workspace_slab_bytes(self._handle._h, L):]
            if workspace.numel() * workspace.element_size() < self.workspace_bytes(frames, L) - 255:
                raise ValueError("workspace too small for that sub-range")
            ws = workspace                   # a slab address: 256-byte alignment is only asked of whole workspaces
        else:
            ws = self._workspace(frames, L, workspace)
        dec = t.empty((frames, n_steps, self.W), dtype=t.int64, device=self.device)
        _lib.check(_lib.load().vit_hip_export_decisions(self._handle._h, _ptr(ws), frames, n_steps, L, _ptr(dec), self._stream()))
        return dec


class DecodePipeline:
    """vit_hip_pipeline_*: a stream of batches through one decoder, scheduled by the library (chainback of batch i beside the
    update of batch i+1, two updates in flight for small batches -- include/vit_hip.h).  The Python face of the C++
    ViterbiDecoder_HIP_Pipeline (include/viterbi_hip/viterbi_decoder_hip_batch.h); the loop it replaces is the reference
    benchmark's per-frame reset -> update -> chainback (examples/run_benchmark.cpp:266-282)."""

    def __init__(self, decoder: BatchDecoder, max_frames: int, L: int, options: "_lib.VitHipPipelineOptions" = None):
        """options: a _lib.VitHipPipelineOptions to override the library's schedule rules (vit_hip_pipeline_create_ex); None: the rules"""
        self.decoder, self.max_frames, self.L = decoder, int(max_frames), int(L)
        self._p = C.c_void_p()
        with decoder.torch.cuda.device(decoder.device):
            if options is None:
                _lib.check(_lib.load().vit_hip_pipeline_create(decoder._handle._h, self.max_frames, self.L, C.byref(self._p)))
            else:
                _lib.check(_lib.load().vit_hip_pipeline_create_ex(decoder._handle._h, self.max_frames, self.L, C.byref(options),
                                                                  C.byref(self._p)))
        self.schedule = _lib.VitHipPipelineSchedule()
        _lib.check(_lib.load().vit_hip_pipeline_get_schedule_v2(self._p, C.byref(self.schedule), C.sizeof(self.schedule)))
        # the pipeline runs on private non-blocking streams: these two events order it against torch's streams
        t = decoder.torch
        with t.cuda.device(decoder.device):
            self._inputs_ready, self._done = t.cuda.Event(), t.cuda.Event()
            self._done.record()                                  # materialises the hipEvent_t the pipeline re-records

    def submit(self, symbols, out, end_state=None, after_current_stream=True):
        """enqueue one batch: symbols [F][L+K-1][R] -> out [F][L/8]; both must stay untouched until sync() / wait_done().
        after_current_stream (default): the batch's update kernel is ordered behind everything already enqueued on torch's
        current stream of the decoder's device (an event recorded there, vit_hip_pipeline_wait_event), so
        `sym = dec.synth(...); pipe.submit(sym, out)` needs no synchronisation in between.  False: the caller guarantees the
        inputs are complete (what a C host without a producer stream does)."""
        t = self.decoder.torch
        frames = self.decoder._check_symbols(symbols, self.L + self.decoder.K - 1)
        if out.dtype != t.uint8 or not out.is_contiguous() or out.numel() != frames * ((self.L + 7) // 8):
            raise ValueError("out must be a contiguous uint8 tensor [frames][ceil(L/8)]")
        L = _lib.load()
        if after_current_stream:
            self._inputs_ready.record(t.cuda.current_stream(self.decoder.device))
            _lib.check(L.vit_hip_pipeline_wait_event(self._p, C.c_void_p(self._inputs_ready.cuda_event)))
        _lib.check(L.vit_hip_pipeline_submit(self._p, _ptr(symbols), frames, _ptr(out), _ptr(end_state), C.c_void_p(self._done.cuda_event)))

    def wait_done(self, stream=None):
        """order `stream` (default: torch's current stream) behind every batch submitted so far, without blocking the host:
        torch work enqueued on it afterwards may read the outputs.  (A later submit(after_current_stream=True) from the same
        stream is then ordered behind these batches too -- call it only where the outputs are consumed.)"""
        t = self.decoder.torch
        (stream or t.cuda.current_stream(self.decoder.device)).wait_event(self._done)

    def sync(self):
        _lib.check(_lib.load().vit_hip_pipeline_sync(self._p))

    def export_last_decisions(self, frames: int = None, n_steps: int = None):
        """decision rows of the most recently submitted (sub-)batch, after sync(): returns (first_frame, rows) where rows
        [n][n_steps][W] belong to frames first_frame .. first_frame + n - 1 of the submitted batch (n = `frames` or the whole
        sub-batch)"""
        dec, t = self.decoder, self.decoder.torch
        n_steps = (self.L + dec.K - 1) if n_steps is None else n_steps
        ws, f0, nf = C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
        _lib.check(_lib.load().vit_hip_pipeline_last_workspace(self._p, C.byref(ws), C.byref(f0), C.byref(nf)))
        n = nf.value if frames is None else min(frames, nf.value)
        out = t.empty((n, n_steps, dec.W), dtype=t.int64, device=dec.device)
        _lib.check(_lib.load().vit_hip_export_decisions(dec._handle._h, ws, n, n_steps, self.L, _ptr(out), dec._stream()))
        return f0.value, out

    def set_timing(self, enable: bool):
        _lib.check(_lib.load().vit_hip_pipeline_set_timing(self._p, 1 if enable else 0))

    def timing(self):
        """(update_ms, chainback_ms, complete_ms) float32 arrays, one entry per batch completed since set_timing(True)"""
        L = _lib.load()
        n = C.c_size_t(0)
        _lib.check(L.vit_hip_pipeline_get_timing(self._p, 0, None, None, None, C.byref(n)))
        u, c, d = (np.zeros(n.value, dtype=np.float32) for _ in range(3))
        _lib.check(L.vit_hip_pipeline_get_timing(self._p, n.value, u.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                                 d.ctypes.data_as(C.c_void_p), C.byref(n)))
        return u, c, d

    def close(self):
        if getattr(self, "_p", None):
            _lib.load().vit_hip_pipeline_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
