// vit_windows.hip -- the windowed decodes of the C ABI: tail-biting frames (vit_hip_decode_tail_biting_batch), one long stream
// (vit_hip_decode_stream) and many lockstep streams (vit_hip_decode_streams).  A layer ABOVE the plans: every route is 1. start
// metrics, 2. the plan's own resumed update, 3. end-state select, 4. the plan's own chainback, 5. the wanted bits cut out -- steps 2
// and 4 through update_batch_impl / chainback_batch_impl (vit_hip.hip) like any outside caller, steps 1, 3 and 5 on the kernels of
// kernels_tb.hpp and kernels_stream.hpp, which only this unit launches.  Host-side logic only: argument checking and launches.
#include "vit_internal.hpp"
#include "kernels_tb.hpp"
#include "kernels_stream.hpp"

using namespace vit;

namespace {
// what the three routes share:
// a caller-owned workspace dealt out part by part, in order, every part 256-byte aligned (include/vit_hip.h)
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += align_up(bytes, 256); return o; }
};

size_t metrics_row_bytes(vit_hip_handle h) { return (size_t)h->N * (size_t)h->error_bytes; }
size_t step_bytes(vit_hip_handle h) { return (size_t)h->R * (size_t)h->soft_bytes; }

// a metric repeated over the four bytes of a dword (u16: twice, u8: four times), as the start-metric kernels store it
uint32_t metric_fill_word(vit_hip_handle h, uint32_t value) {
    return h->error_bytes == 2 ? (value & 0xFFFFu) * 0x00010001u : (value & 0xFFu) * 0x01010101u;
}

// a window's warm-up in front and behind spans at least the code's memory
const char* extension_invalid(vit_hip_handle h, size_t head, size_t tail) {
    return head < (size_t)h->K - 1 || tail < (size_t)h->K - 1 ? "head and tail must be >= K-1" : nullptr;
}

// the caller's buffers of a decode call, `need` the size of its workspace layout
int check_buffers(vit_hip_handle h, const void* d_symbols, const void* d_workspace, size_t workspace_bytes, size_t need, const void* d_bytes_out) {
    if (!d_symbols || !d_workspace || !d_bytes_out) return fail(VIT_HIP_ERR_INVALID_ARG, "d_symbols/d_workspace/d_bytes_out is NULL");
    if (h->soft_bytes == 2 && misaligned(d_symbols, 2)) return fail(VIT_HIP_ERR_INVALID_ARG, "int16 symbols must be 2-byte aligned");
    if (workspace_bytes < need) return fail(VIT_HIP_ERR_WORKSPACE, "workspace too small");
    if (misaligned(d_workspace, 256)) return fail(VIT_HIP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    return VIT_HIP_OK;
}

// step 3 of every route: end_ws[f] (and end_out[f], when asked for) = the state of frame f's smallest final metric.  With a
// keep_period the frames f % keep_period == keep_phase keep the end state they hold (kernels_tb.hpp).  No frames: no launch
int select_end_states(vit_hip_handle h, const char* route, hipStream_t st, const void* metrics, uint32_t* end_ws, uint32_t* end_out,
                      size_t frames, size_t keep_period = 0, size_t keep_phase = 0) {
    if (frames == 0) return VIT_HIP_OK;
    vit::TbSelectArgs s{};
    s.metrics = metrics; s.end_ws = end_ws; s.end_out = end_out;
    s.frames = (uint32_t)frames; s.log2N = (uint32_t)(h->K - 1);
    s.keep_period = (uint32_t)keep_period; s.keep_phase = (uint32_t)keep_phase;
    if (vit::tb_launch_select(h->error_bytes, s, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, std::string(route) + " end-state launch failed");
    return VIT_HIP_OK;
}

// the caller-owned workspace of one tail-biting call
struct TbLayout {
    size_t S_ext, L_ext, nbe;                      // extended steps, extended chainback bits, its bytes per frame
    size_t dec, ext, met, end, bytes, total;       // offsets, and the whole size
};

// argument rule of the tail-biting entry points: L >= K, head and tail >= K-1, and sizes the launchers' 32-bit counters hold
const char* tb_invalid(vit_hip_handle h, size_t frames, size_t L, size_t head, size_t tail) {
    if (L < (size_t)h->K) return "tail-biting frames need L >= K";
    if (const char* why = extension_invalid(h, head, tail)) return why;
    if (frames > 0x7FFFFFF0u || L > 0x10000000u || head > 0x10000000u || tail > 0x10000000u) return "batch too large";
    return nullptr;
}

TbLayout tb_layout(vit_hip_handle h, size_t frames, size_t L, size_t head, size_t tail) {
    TbLayout o;
    o.S_ext = head + L + tail;
    o.L_ext = o.S_ext - ((size_t)h->K - 1);
    o.nbe = (o.L_ext + 7) / 8;
    Carve ws;
    o.dec = ws.take(vit_hip_workspace_bytes(h, frames, o.L_ext));      // the plan's decisions over the extension
    o.ext = ws.take(frames * o.S_ext * step_bytes(h));                 // the extended symbols
    o.met = ws.take(frames * metrics_row_bytes(h));
    o.end = ws.take(frames * sizeof(uint32_t));
    o.bytes = ws.take(frames * o.nbe);                                 // the chainback over the extension
    o.total = ws.at;
    return o;
}

// the windows of one vit_hip_decode_stream / vit_hip_decode_streams call and its caller-owned workspace.  One stream is
// n_streams = 1: rows_u = n_u and one remainder frame, what vit_hip_decode_stream always laid out.
struct StreamLayout {
    size_t a = 0, b = 0, n = 0, n_u = 0;           // per stream: emitted range [a, b), windows, of which uniform (n_u == n or n - 1)
    size_t S_u = 0, L_u = 0, nbe_u = 0;            // a uniform window's steps, chainback bits, bytes
    size_t S_r = 0, L_r = 0, nbe_r = 0;            // the remainder window's (0 when every window has the same length)
    size_t n_streams = 1, period = 0;              // streams; grid windows from one stream's window 0 to the next one's (pitch / W)
    size_t rows_u = 0, rows_r = 0;                 // launched grid windows (n_streams - 1) * period + n_u; remainder frames
    size_t dec_u = 0, dec_r = 0, met_u = 0, met_r = 0, end_u = 0, end_r = 0, bytes_u = 0, bytes_r = 0, total = 0;
};

// argument rule of the stream entry points; fills the window bookkeeping of `o` when the arguments pass
const char* stream_invalid(vit_hip_handle h, size_t T, size_t W, size_t head, size_t tail, unsigned flags, StreamLayout& o) {
    const size_t K = (size_t)h->K;
    const bool begin = flags & VIT_HIP_STREAM_BEGIN, end = flags & VIT_HIP_STREAM_END;
    if (flags & ~(unsigned)(VIT_HIP_STREAM_BEGIN | VIT_HIP_STREAM_END)) return "unknown stream flags";
    if (const char* why = extension_invalid(h, head, tail)) return why;
    if (W < 8 || W < head || W < tail) return "the window must be >= 8, >= head and >= tail";
    if (T > 0x7FFFFFF0u || W > 0x10000000u) return "segment too large";
    if (T < head + tail + (begin ? 0 : 1)) return "the segment must hold head + tail steps (and one more without BEGIN)";
    o.a = begin ? 0 : head;
    o.b = end ? T - (K - 1) : T - tail;
    if (o.b <= o.a) return "the segment emits no bit";
    // b > a >= 0 and T >= head + tail; b >= head: END: T - (K-1) >= head + tail - (K-1) >= head; else T - tail >= head
    o.n = (o.b - head) / W;
    if (o.n < 1) o.n = 1;
    o.S_u = head + W + tail;
    const size_t last = T - (o.n - 1) * W;          // steps of the last window
    o.n_u = last == o.S_u ? o.n : o.n - 1;
    o.S_r = o.n_u == o.n ? 0 : last;
    // the register plan addresses a tile's symbols through 32-bit offsets with the sign bit kept free (reg_update): the last of a
    // tile's (at most 128) overlapped windows ends (tile - 1) * W + S_u steps into it; the remainder window is one frame
    if ((127 * W + o.S_u) * step_bytes(h) + 65536 >= 0x7FFF0000ull || o.S_r * step_bytes(h) + 65536 >= 0x7FFF0000ull)
        return "window too large for the launchers' 32-bit symbol offsets";
    o.n_streams = 1;
    o.period = 0;
    o.rows_u = o.n_u;
    o.rows_r = o.S_r ? 1 : 0;
    return nullptr;
}

// the same for n_streams lockstep streams `pitch` steps apart: each stream under the rule above, all of them on one grid of W steps
const char* streams_invalid(vit_hip_handle h, size_t n_streams, size_t pitch, size_t T, size_t W, size_t head, size_t tail, unsigned flags,
                            StreamLayout& o) {
    if (const char* why = stream_invalid(h, T, W, head, tail, flags, o)) return why;
    if (n_streams < 1 || n_streams > 0x7FFFFFF0u) return "n_streams must be >= 1 (and within the launchers' batch limit)";
    if (pitch < T || pitch % W != 0) return "pitch must be >= T and a multiple of the window";
    o.n_streams = n_streams;
    o.period = pitch / W;                           // > n_u, >= n: the last window of a stream ends inside its pitch
    // no useful window on the grid (every stream is one remainder window): the grid is not launched
    o.rows_u = o.n_u ? (n_streams - 1) * o.period + o.n_u : 0;
    o.rows_r = o.S_r ? n_streams : 0;
    if (o.rows_u > 0x7FFFFFF0u) return "too many windows for one batch";
    // the remainder windows are a batch at stride pitch: a register-plan tile of them spans tile * pitch steps (reg_update's bound)
    const size_t tile = h->plan == VIT_HIP_PLAN_REG ? (size_t)h->reg_code.tile : 1;
    if (o.rows_r > 1 && pitch * step_bytes(h) * tile + 65536 >= 0x7FFF0000ull) return "pitch too large for the launchers' 32-bit symbol offsets";
    return nullptr;
}

// fills the workspace layout of `o` and returns its size
size_t stream_layout(vit_hip_handle h, StreamLayout& o) {
    const size_t K1 = (size_t)h->K - 1;
    o.L_u = o.S_u - K1;
    o.nbe_u = (o.L_u + 7) / 8;
    o.L_r = o.S_r ? o.S_r - K1 : 0;
    o.nbe_r = (o.L_r + 7) / 8;
    Carve ws;
    o.dec_u = ws.take(o.rows_u ? vit_hip_workspace_bytes(h, o.rows_u, o.L_u) : 0);     // the plan's decisions: the grid windows,
    o.dec_r = ws.take(o.rows_r ? vit_hip_workspace_bytes(h, o.rows_r, o.L_r) : 0);     // the remainder windows
    o.met_u = ws.take(o.rows_u * metrics_row_bytes(h));
    o.met_r = ws.take(o.rows_r * metrics_row_bytes(h));
    o.end_u = ws.take(o.rows_u * sizeof(uint32_t));
    o.end_r = ws.take(o.rows_r * sizeof(uint32_t));
    // the chainback rows, 16 bytes of slack behind each part: the stitch kernel's loads stay inside the rows, this keeps them off the
    // next part anyway
    o.bytes_u = ws.take(o.rows_u * o.nbe_u + 16);
    o.bytes_r = ws.take(o.rows_r * o.nbe_r + 16);
    return o.total = ws.at;
}

// what both decode entry points do once their argument rule has passed: the buffer checks, the launches, n_bits_out.
// pitch and out_pitch: unused with one stream
int decode_streams_checked(vit_hip_handle h, StreamLayout& lay, const void* d_symbols, size_t pitch, size_t W, size_t head, unsigned flags,
                           void* d_workspace, size_t workspace_bytes, uint8_t* d_bytes_out, size_t out_pitch, size_t* n_bits_out,
                           vit_hip_stream_t stream) {
    const size_t need = stream_layout(h, lay);
    if (const int rc = check_buffers(h, d_symbols, d_workspace, workspace_bytes, need, d_bytes_out); rc != VIT_HIP_OK) return rc;
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool begin = flags & VIT_HIP_STREAM_BEGIN, end = flags & VIT_HIP_STREAM_END;
    const bool rem = lay.S_r != 0, many = lay.n_streams > 1;
    uint8_t* ws = (uint8_t*)d_workspace;
    void *met_u = ws + lay.met_u, *met_r = ws + lay.met_r;
    uint32_t *end_u = (uint32_t*)(ws + lay.end_u), *end_r = (uint32_t*)(ws + lay.end_r);

    // 1. the start metrics of every window, and end state 0 for the last one of every stream under END
    vit::StreamInitArgs in{};
    in.met_u = met_u; in.met_r = met_r;
    if (end) {
        in.end_zero = rem ? end_r : end_u + (lay.n_u - 1);
        in.end_zero_count = (uint32_t)lay.n_streams;
        in.end_zero_stride = (uint32_t)(rem ? 1 : lay.period);
    }
    in.bytes_u = lay.rows_u * metrics_row_bytes(h);
    in.bytes_r = lay.rows_r * metrics_row_bytes(h);
    in.chunks_u = (in.bytes_u + 15) / 16;
    in.total_chunks = in.chunks_u + (in.bytes_r + 15) / 16;
    in.row_bytes = (uint32_t)metrics_row_bytes(h);
    in.row_shift = (uint32_t)(h->K - 1) + (h->error_bytes == 2 ? 1u : 0u);
    in.fill = metric_fill_word(h, h->cfg_raw[1]);
    in.non_start = metric_fill_word(h, h->cfg_raw[2]);
    // window 0 of a stream is row s * period of the grid; with one stream row 0 alone (a period no other row reaches)
    in.begin_period_u = !begin || !lay.rows_u ? 0u : (uint32_t)(many ? lay.period : lay.rows_u);
    in.begin_r = begin && !lay.n_u ? 1u : 0u;
    if (vit::stream_launch_init(h->error_bytes, in, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "stream init launch failed");

    // 2. the plan's own update, resumed in place from those metrics: the grid windows as one batch whose frame stride is W steps of
    //    the caller's buffer (the windows overlap; nothing is gathered), then the longer last windows as a batch of one frame per
    //    stream at stride pitch.  Here and in 4. a batch of no windows (rows_u or rows_r == 0) launches nothing
    if (const int rc = update_batch_impl(h, d_symbols, W * (size_t)h->R, lay.rows_u, 0, lay.S_u, lay.L_u, ws + lay.dec_u, lay.dec_r - lay.dec_u,
                                         met_u, met_u, nullptr, nullptr, stream, true); rc != VIT_HIP_OK) return rc;
    if (const int rc = update_batch_impl(h, (const uint8_t*)d_symbols + (lay.n - 1) * W * step_bytes(h), many ? pitch * (size_t)h->R : 0,
                                         lay.rows_r, 0, lay.S_r, lay.L_r, ws + lay.dec_r, lay.met_u - lay.dec_r, met_r, met_r, nullptr,
                                         nullptr, stream); rc != VIT_HIP_OK) return rc;

    // 3. end state = smallest final metric, for every window but the last one of a stream under END: the grid's last row is left out
    //    of the launch, the other streams' last rows keep their 0 (keep_period)
    const bool zero_u = end && !rem;
    if (const int rc = select_end_states(h, "stream", st, met_u, end_u, nullptr, lay.rows_u - (zero_u && lay.rows_u ? 1 : 0),
                                         zero_u && many ? lay.period : 0, zero_u && many ? lay.n_u - 1 : 0); rc != VIT_HIP_OK) return rc;
    if (const int rc = select_end_states(h, "stream", st, met_r, end_r, nullptr, end ? 0 : lay.rows_r); rc != VIT_HIP_OK) return rc;

    // 4. the plan's own chainback of every window over all its steps, from those states
    if (const int rc = chainback_batch_impl(h, ws + lay.dec_u, lay.rows_u, lay.L_u, ws + lay.bytes_u, end_u, stream, 0); rc != VIT_HIP_OK) return rc;
    if (const int rc = chainback_batch_impl(h, ws + lay.dec_r, lay.rows_r, lay.L_r, ws + lay.bytes_r, end_r, stream, 0); rc != VIT_HIP_OK) return rc;

    // 5. each window's share of the output, as one bit stream per stream; the bridge windows' rows are not read
    vit::StreamStitchArgs w{};
    w.rows_u = ws + lay.bytes_u;
    w.row_r = ws + lay.bytes_r;
    w.out = d_bytes_out;
    w.out_pitch = many ? out_pitch : 0;
    w.n_streams = (uint32_t)lay.n_streams;
    w.period = (uint32_t)lay.period;
    w.nb = (lay.b - lay.a + 7) / 8;
    w.chunks = (w.nb + 15) / 16;
    w.a = (uint32_t)lay.a; w.b = (uint32_t)lay.b;
    w.n = (uint32_t)lay.n; w.n_u = (uint32_t)lay.n_u;
    w.W = (uint32_t)W; w.head = (uint32_t)head;
    w.nbe_u = (uint32_t)lay.nbe_u; w.nbe_r = (uint32_t)lay.nbe_r;
    w.out_aligned = ((uintptr_t)d_bytes_out & 15u) == 0 && (w.out_pitch & 15u) == 0 ? 1u : 0u;
    if (vit::stream_launch_stitch(w, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "stream stitch launch failed");
    if (n_bits_out) *n_bits_out = lay.b - lay.a;
    return VIT_HIP_OK;
}
}  // namespace

extern "C" {

size_t vit_hip_tail_biting_workspace_bytes(vit_hip_handle h, size_t frames, size_t L, size_t head, size_t tail) {
    return !h || tb_invalid(h, frames, L, head, tail) ? 0 : tb_layout(h, frames, L, head, tail).total;
}

int vit_hip_decode_tail_biting_batch(vit_hip_handle h, const void* d_symbols, size_t frames, size_t L, size_t head, size_t tail,
                                     void* d_workspace, size_t workspace_bytes, uint8_t* d_bytes_out, uint32_t* d_end_state_out,
                                     uint8_t* d_tail_biting_ok, vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (const char* why = tb_invalid(h, frames, L, head, tail)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    const TbLayout lay = tb_layout(h, frames, L, head, tail);
    if (const int rc = check_buffers(h, d_symbols, d_workspace, workspace_bytes, lay.total, d_bytes_out); rc != VIT_HIP_OK) return rc;
    if (frames == 0) return VIT_HIP_OK;
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)d_workspace;
    void *ext = ws + lay.ext, *met = ws + lay.met;
    uint32_t* end = (uint32_t*)(ws + lay.end);
    uint8_t* ext_bytes = ws + lay.bytes;

    // 1. the extended symbols and every state a start state
    vit::TbGatherArgs g{};
    g.symbols = d_symbols; g.ext = ext; g.metrics = met;
    g.ext_elems = (uint64_t)frames * lay.S_ext * (uint64_t)h->R;
    g.gather_chunks = (g.ext_elems * (uint64_t)h->soft_bytes + 15) / 16;
    g.metric_bytes = (uint64_t)frames * metrics_row_bytes(h);
    g.total_chunks = g.gather_chunks + (g.metric_bytes + 15) / 16;
    g.L = (uint32_t)L; g.R = (uint32_t)h->R; g.S_ext = (uint32_t)lay.S_ext;
    g.shift = (uint32_t)((L - head % L) % L);
    g.fill = metric_fill_word(h, h->cfg_raw[1]);
    if (vit::tb_launch_gather(h->soft_bytes, g, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "tail-biting gather launch failed");

    // 2. the plan's own update over the whole extension, resumed in place from those metrics (every plan resumes: PLAN_LDS in place)
    if (const int rc = update_batch_impl(h, ext, 0, frames, 0, lay.S_ext, lay.L_ext, ws + lay.dec, lay.ext - lay.dec, met, met, nullptr, nullptr,
                                         stream); rc != VIT_HIP_OK) return rc;

    // 3. end state = smallest final metric
    if (const int rc = select_end_states(h, "tail-biting", st, met, end, d_end_state_out, frames); rc != VIT_HIP_OK) return rc;

    // 4. the plan's own chainback over the extension from those states
    if (const int rc = chainback_batch_impl(h, ws + lay.dec, frames, lay.L_ext, ext_bytes, end, stream, 0); rc != VIT_HIP_OK) return rc;

    // 5. the window [head, head + L) and the tail-biting flag
    vit::TbWindowArgs w{};
    w.ext_bytes = ext_bytes; w.out = d_bytes_out; w.ok = d_tail_biting_ok;
    w.nbe = (uint32_t)lay.nbe;
    w.nb = (uint32_t)((L + 7) / 8);
    w.total = (uint64_t)frames * w.nb;
    w.L = (uint32_t)L; w.head = (uint32_t)head; w.K = (uint32_t)h->K;
    if (vit::tb_launch_window(w, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "tail-biting window launch failed");
    return VIT_HIP_OK;
}

size_t vit_hip_stream_workspace_bytes(vit_hip_handle h, size_t T, size_t W, size_t head, size_t tail, unsigned flags) {
    StreamLayout lay;
    return !h || stream_invalid(h, T, W, head, tail, flags, lay) ? 0 : stream_layout(h, lay);
}

int vit_hip_decode_stream(vit_hip_handle h, const void* d_symbols, size_t T, size_t W, size_t head, size_t tail, unsigned flags,
                          void* d_workspace, size_t workspace_bytes, uint8_t* d_bytes_out, size_t* n_bits_out,
                          vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    StreamLayout lay;
    if (const char* why = stream_invalid(h, T, W, head, tail, flags, lay)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    return decode_streams_checked(h, lay, d_symbols, 0, W, head, flags, d_workspace, workspace_bytes, d_bytes_out, 0, n_bits_out, stream);
}

size_t vit_hip_streams_workspace_bytes(vit_hip_handle h, size_t n_streams, size_t pitch, size_t T, size_t W, size_t head, size_t tail,
                                       unsigned flags) {
    StreamLayout lay;
    return !h || streams_invalid(h, n_streams, pitch, T, W, head, tail, flags, lay) ? 0 : stream_layout(h, lay);
}

int vit_hip_decode_streams(vit_hip_handle h, const void* d_symbols, size_t n_streams, size_t pitch, size_t T, size_t W, size_t head,
                           size_t tail, unsigned flags, void* d_workspace, size_t workspace_bytes, uint8_t* d_bytes_out,
                           size_t out_pitch_bytes, size_t* n_bits_out, vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    StreamLayout lay;
    if (const char* why = streams_invalid(h, n_streams, pitch, T, W, head, tail, flags, lay)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (out_pitch_bytes < (lay.b - lay.a + 7) / 8) return fail(VIT_HIP_ERR_INVALID_ARG, "out_pitch_bytes shorter than ceil(n_out/8)");
    return decode_streams_checked(h, lay, d_symbols, pitch, W, head, flags, d_workspace, workspace_bytes, d_bytes_out, out_pitch_bytes,
                                  n_bits_out, stream);
}

}  // extern "C"
