// vit_sync.hip -- node synchronisation of the C ABI: vit_hip_sync_build (one received buffer -> the stream of every alignment
// hypothesis) and vit_hip_sync_search (build, decode, re-encode, count, rank in one call).  A layer ABOVE the windowed decode and the
// channel symbol error count: those run through their own entry points (vit_hip_decode_streams of vit_windows.hip, the body of
// vit_hip_channel_errors_batch of vit_encode.hip, whose counters the start-state kernel zeroes so that the call enqueues kernels only); the kernels of kernels_sync.hpp, which only this unit
// launches, are the front end, the start states and the ranking.  Host-side logic only: argument checking and launches.
#include "vit_internal.hpp"
#include "kernels_sync.hpp"

using namespace vit;

namespace {

constexpr unsigned SYNC_FLAGS = VIT_HIP_SYNC_SWAP_PAIRS | VIT_HIP_SYNC_NEGATE_EVEN | VIT_HIP_SYNC_NEGATE_ODD;

// the puncturing scheme of a call: NULL / 0 / 0 is the identity over one trellis step
struct SyncMap {
    const int32_t* d_source_index;
    size_t period, kept;
};

// argument rule of the build (include/vit_hip.h): everything the host can know without reading device memory
const char* build_invalid(vit_hip_handle h, size_t n_received, SyncMap& m, const vit_hip_sync_hypothesis* hyp, size_t n_hyp, size_t T) {
    const size_t R = (size_t)h->R;
    if (!m.d_source_index) {
        if (m.period != 0 || m.kept != 0) return "without a source map period_symbols and kept_per_period must be 0";
        m.period = m.kept = R;
    } else {
        if (m.period == 0 || m.period % R != 0) return "period_symbols must be a positive multiple of R";
        if (m.kept == 0 || m.kept > m.period) return "kept_per_period must be 1 .. period_symbols";
        if (m.period > 0x7FFFFFFFu) return "period_symbols too large";
    }
    if (!hyp || n_hyp < 1 || n_hyp > SYNC_MAX_HYPOTHESES) return "1 to 64 hypotheses per call";
    if (T == 0 || T >= 0x100000000ull / R) return "T * R must be 1 .. 2^32 - 1";
    const size_t n = T * R, full = n / m.period, rem = n % m.period;
    // the received symbols a hypothesis needs: whole periods read all their kept symbols; of the last, partial one the host knows
    // the map only when it is the identity -- otherwise it is counted as if it read the period's last kept symbol
    const size_t span = full * m.kept + (rem == 0 ? 0 : m.d_source_index ? m.kept : rem);
    for (size_t i = 0; i < n_hyp; ++i) {
        if (hyp[i].flags & ~SYNC_FLAGS) return "unknown hypothesis flag bits";
        size_t last = (size_t)hyp[i].offset + span - 1;                  // the largest j read
        if (hyp[i].flags & VIT_HIP_SYNC_SWAP_PAIRS) last |= 1;           // j ^ 1 of the pair it lies in
        if (last >= n_received) return "a hypothesis reads past n_received";
    }
    return nullptr;
}

int launch_build(vit_hip_handle h, const void* d_received, const SyncMap& m, const vit_hip_sync_hypothesis* hyp, size_t n_hyp, size_t T,
                 size_t pitch, void* d_out, hipStream_t st) {
    SyncBuildArgs a{};
    a.received = d_received;
    a.source_index = m.d_source_index;
    a.out = d_out;
    a.out_stride = (uint64_t)pitch * (uint64_t)h->R;
    a.n_elems = (uint32_t)(T * (size_t)h->R);
    a.period = (uint32_t)m.period; a.kept = (uint32_t)m.kept;
    a.mid = h->high + h->low;
    for (size_t i = 0; i < n_hyp; ++i) a.hyp[i] = hyp[i];
    if (sync_launch_build(h->soft_bytes, a, (uint32_t)n_hyp, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "sync build launch failed");
    return VIT_HIP_OK;
}

const char* buffers_invalid(vit_hip_handle h, const void* d_received, const void* d_out) {
    if (!d_received || !d_out) return "NULL buffer";
    if (h->soft_bytes == 2 && (misaligned(d_received, 2) || misaligned(d_out, 2))) return "int16 symbols must be 2-byte aligned";
    return nullptr;
}

// the caller-owned workspace of one search, every part 256-byte aligned: the hypothesis streams on the window grid, their decoded
// bytes, the start states of the re-encoding, then the workspace of vit_hip_decode_streams
struct SearchLayout {
    size_t pitch, n_out, skip, out_pitch;
    size_t sym, bytes, state, decode, decode_bytes, total;
};

const char* search_invalid(vit_hip_handle h, size_t n_hyp, size_t T, size_t W, size_t head, size_t tail, SearchLayout& o) {
    if (n_hyp < 1 || n_hyp > SYNC_MAX_HYPOTHESES) return "1 to 64 hypotheses per call";
    if (W == 0 || T == 0 || T > 0x7FFFFFF0u) return "T and W must be positive (and T within the stream limit)";
    o.pitch = (T + W - 1) / W * W;
    o.decode_bytes = vit_hip_streams_workspace_bytes(h, n_hyp, o.pitch, T, W, head, tail, 0);
    if (o.decode_bytes == 0) return "T, W, head, tail outside the rule of vit_hip_decode_streams";
    o.n_out = T - head - tail;
    o.skip = 8 * (((size_t)h->K - 1 + 7) / 8);
    if (o.n_out <= o.skip) return "the segment must emit more than 8 * ceil((K-1)/8) bits";
    o.out_pitch = align_up((o.n_out + 7) / 8, 16);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t off = at; at += align_up(bytes, 256); return off; };
    o.sym = take(n_hyp * o.pitch * (size_t)h->R * (size_t)h->soft_bytes);
    o.bytes = take(n_hyp * o.out_pitch);
    o.state = take(n_hyp * sizeof(uint32_t));
    o.decode = take(o.decode_bytes);
    o.total = at;
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_sync_build(vit_hip_handle h, const void* d_received, size_t n_received, const int32_t* d_source_index, size_t period_symbols,
                       size_t kept_per_period, const vit_hip_sync_hypothesis* hypotheses, size_t n_hyp, size_t T, size_t pitch,
                       void* d_symbols_out, vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    SyncMap m{d_source_index, period_symbols, kept_per_period};
    if (const char* why = build_invalid(h, n_received, m, hypotheses, n_hyp, T)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (pitch < T) return fail(VIT_HIP_ERR_INVALID_ARG, "pitch must be >= T");
    if (const char* why = buffers_invalid(h, d_received, d_symbols_out)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    VIT_HIP_ON_DEVICE(h->device);
    return launch_build(h, d_received, m, hypotheses, n_hyp, T, pitch, d_symbols_out, (hipStream_t)stream);
}

size_t vit_hip_sync_search_workspace_bytes(vit_hip_handle h, size_t n_hyp, size_t T, size_t W, size_t head, size_t tail) {
    SearchLayout lay;
    return !h || !h->linear || search_invalid(h, n_hyp, T, W, head, tail, lay) ? 0 : lay.total;
}

int vit_hip_sync_search(vit_hip_handle h, const void* d_received, size_t n_received, const int32_t* d_source_index, size_t period_symbols,
                        size_t kept_per_period, const vit_hip_sync_hypothesis* hypotheses, size_t n_hyp, size_t T, size_t W, size_t head,
                        size_t tail, void* d_workspace, size_t workspace_bytes, uint32_t* d_errors, uint32_t* d_compared, uint32_t* d_best,
                        vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (!h->linear) return fail(VIT_HIP_ERR_UNSUPPORTED, "the branch table is not that of a convolutional code (no polynomials)");
    SearchLayout lay;
    if (const char* why = search_invalid(h, n_hyp, T, W, head, tail, lay)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    SyncMap m{d_source_index, period_symbols, kept_per_period};
    if (const char* why = build_invalid(h, n_received, m, hypotheses, n_hyp, T)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (!d_errors || !d_compared) return fail(VIT_HIP_ERR_INVALID_ARG, "d_errors / d_compared is NULL");
    if (!d_workspace) return fail(VIT_HIP_ERR_INVALID_ARG, "d_workspace is NULL");
    if (const char* why = buffers_invalid(h, d_received, d_workspace)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (workspace_bytes < lay.total) return fail(VIT_HIP_ERR_WORKSPACE, "workspace too small");
    if (misaligned(d_workspace, 256)) return fail(VIT_HIP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)d_workspace;
    uint8_t* sym = ws + lay.sym;
    uint8_t* bytes = ws + lay.bytes;
    uint32_t* state = (uint32_t*)(ws + lay.state);
    const size_t step_bytes = (size_t)h->R * (size_t)h->soft_bytes;

    // 1. the hypothesis streams, `pitch` steps apart on one window grid
    if (const int rc = launch_build(h, d_received, m, hypotheses, n_hyp, T, lay.pitch, sym, st); rc != VIT_HIP_OK) return rc;

    // 2. every stream decoded as a mid-stream segment: bits of steps [head, T - tail)
    if (const int rc = vit_hip_decode_streams(h, sym, n_hyp, lay.pitch, T, W, head, tail, 0, ws + lay.decode, lay.decode_bytes, bytes,
                                              lay.out_pitch, nullptr, stream); rc != VIT_HIP_OK) return rc;

    // 3. the encoder state in front of emitted bit `skip`: the K-1 bits before it; the same threads zero the counters step 4 adds into
    SyncStateArgs s{};
    s.bytes = bytes; s.state = state; s.errors = d_errors; s.compared = d_compared; s.byte_stride = lay.out_pitch;
    s.n_hyp = (uint32_t)n_hyp; s.skip_bytes = (uint32_t)(lay.skip / 8); s.K = (uint32_t)h->K;
    if (sync_launch_state(s, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "sync state launch failed");

    // 4. the bits from `skip` on, encoded again from that state, against the hypothesis's own symbols
    if (const int rc = channel_errors_impl(h, sym + (head + lay.skip) * step_bytes, lay.pitch * (size_t)h->R, bytes + lay.skip / 8,
                                           lay.out_pitch, n_hyp, lay.n_out - lay.skip, 0, state, d_errors, d_compared, false, stream);
        rc != VIT_HIP_OK) return rc;

    // 5. the hypothesis no other beats
    if (d_best) {
        SyncPickArgs p{};
        p.errors = d_errors; p.compared = d_compared; p.best = d_best; p.n_hyp = (uint32_t)n_hyp;
        if (sync_launch_pick(p, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "sync pick launch failed");
    }
    return VIT_HIP_OK;
}

}  // extern "C"
