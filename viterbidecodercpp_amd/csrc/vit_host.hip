// vit_host.hip -- the routes of ONE decoder object whose state lives on the host between calls: vit_hip_update_host /
// vit_hip_chainback_host (every call stages through pinned memory) and the frame route (vit_hip_update_host_lazy /
// vit_hip_chainback_host_lazy / vit_hip_fetch_decisions_host: rows kept on the device, one launch per frame).  K <= 7, and K = 8, 9
// with R <= 4, run the single-frame kernels of kernels_one.hpp, which only this unit launches; larger codes -- and any code after
// vit_hip_set_host_route(h, VIT_HIP_HOST_ROUTE_LDS) -- the LDS plan on one frame (vit_hip.hip).
#include "vit_internal.hpp"
#include "kernels_one.hpp"

using namespace vit;

namespace {

// the handle's device scratch and its pinned host stage, both at least `bytes` (grown with headroom, contents not kept)
int ensure_scratch_and_stage(vit_hip_handle h, size_t bytes) {
    const size_t want = bytes + bytes / 2 + 4096;
    auto grow = [&](void*& p, size_t& have, bool pinned) -> int {
        if (bytes <= have) return VIT_HIP_OK;
        if (p) VIT_HIP_CHECK(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; have = 0;
        VIT_HIP_CHECK(pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want));
        have = want;
        return VIT_HIP_OK;
    };
    const int rc = grow(h->d_scratch, h->scratch_bytes, false);
    return rc != VIT_HIP_OK ? rc : grow(h->h_stage, h->stage_bytes, true);
}

// frame route: the device row store holds rows [0, rows) of the frame (contents kept when it grows)
int ensure_rows(vit_hip_handle h, size_t rows) {
    if (rows <= h->rows_cap) return VIT_HIP_OK;
    const size_t want = rows + rows / 2 + 64;
    uint64_t* p = nullptr;
    VIT_HIP_CHECK(hipMalloc((void**)&p, want * (size_t)h->W * 8));
    if (h->d_rows) {
        VIT_HIP_CHECK(hipStreamSynchronize(h->stream));
        if (hipMemcpy(p, h->d_rows, h->rows_cap * (size_t)h->W * 8, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(p); return fail(VIT_HIP_ERR_RUNTIME, "row store copy failed"); }
        (void)hipFree(h->d_rows);
    }
    h->d_rows = p;
    h->rows_cap = want;
    return VIT_HIP_OK;
}

int ensure_map(vit_hip_handle h, size_t bytes) {
    if (bytes <= h->map_bytes) return VIT_HIP_OK;
    VIT_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (h->h_map) VIT_HIP_CHECK(hipHostFree(h->h_map));
    h->h_map = nullptr;
    h->map_bytes = 0;
    h->spec_valid = false;
    const size_t want = bytes + bytes / 2 + 4096;
    VIT_HIP_CHECK(hipHostMalloc(&h->h_map, want, hipHostMallocMapped | hipHostMallocCoherent));
    memset(h->h_map, 0, 256);
    h->map_bytes = want;
    return VIT_HIP_OK;
}

// ---- launchers of the single-frame kernels (kernels_one.hpp) ----
template <int SHIFT>
int one_launch_update(int R, const OneUpdateArgs& a, hipStream_t st) {
    return with_rate(R, -1, [&](auto r) {
        if constexpr (r() <= 4) {
            if (one_update7_supported(a.K, r())) {
                hipLaunchKernelGGL((one_update7_kernel<r(), SHIFT>), dim3(1), dim3(192), 0, st, a);
                return hipGetLastError() == hipSuccess ? 0 : -1;
            }
        }
        hipLaunchKernelGGL((one_update_kernel<r(), SHIFT>), dim3(1), dim3(64), 0, st, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

template <int SHIFT>
int one_launch_frame(int R, const OneFrameArgs& a, hipStream_t st) {
    const size_t smem = a.do_chainback ? one_chainback_lds_bytes() : 0;
    auto launch = [&](auto kern, unsigned threads, size_t static_limit) {
        if (smem > static_limit && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return -1;
        hipLaunchKernelGGL(kern, dim3(1), dim3(threads), smem, st, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    };
    return with_rate(R, -1, [&](auto r) {
        if constexpr (r() <= 4) {
            if (one_update7_supported(a.u.K, r())) return launch(one_frame7_kernel<r(), SHIFT>, 192u, 32 * 1024);
        }
        return launch(one_frame_kernel<r(), SHIFT>, 64u, 64 * 1024);
    });
}

// (K = 8, 9 with R <= 4: the launchers of the wide kernels are vit_host_wide.hip's, declared in kernels_one.hpp)

// which kernels serve this handle's single-decoder routes (vit_hip_host_route_note names them)
enum HostFamily { HOST_ONE7, HOST_ONE, HOST_WIDE, HOST_LDS };
HostFamily host_family(vit_hip_handle h) {
    if (h->host_route == VIT_HIP_HOST_ROUTE_LDS) return HOST_LDS;
    if (one_update7_supported(h->K, h->R)) return HOST_ONE7;
    if (one_supported(h->K, h->R)) return HOST_ONE;
    if (one_wide_supported(h->K, h->R)) return HOST_WIDE;
    return HOST_LDS;
}

// K <= 9: rows staged through LDS by the whole wavefront, 64 segments chased at once (kernels_one.hpp); the end state is a kernel argument
int one_launch_chainback(vit_hip_handle h, const uint64_t* d_rows, size_t L, size_t end_state, uint8_t* d_out) {
    if (L > 0xFFFFFFF0ull) return fail(VIT_HIP_ERR_INVALID_ARG, "L too large");
    OneChainbackArgs ca{};
    ca.decisions = d_rows;
    ca.out = d_out;
    ca.end_state = (uint32_t)end_state;
    ca.L = (uint32_t)L;
    ca.K = h->K;
    // per launch, like every other > 64 KiB launcher of the library: the attribute belongs to the CURRENT device's function object
    // (a process-wide `static` would opt in only the device of the first caller: a decoder on device 1..7 launched without it)
    if (h->W > 1) {
        VIT_HIP_CHECK(one_wide_launch_chainback(h->W, ca, h->stream));
        return VIT_HIP_OK;
    }
    VIT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(one_chainback_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)one_chainback_lds_bytes()));
    hipLaunchKernelGGL(one_chainback_kernel, dim3(1), dim3(64), one_chainback_lds_bytes(), h->stream, ca);
    VIT_HIP_CHECK(hipGetLastError());
    return VIT_HIP_OK;
}

// chainback of the one frame whose rows are on the device: the single-frame kernel, or the LDS plan with the end state in d_end_state
int chainback_one_frame(vit_hip_handle h, const uint64_t* d_rows, size_t L, size_t end_state, uint8_t* d_out, uint32_t* d_end_state) {
    if (host_family(h) != HOST_LDS) return one_launch_chainback(h, d_rows, L, end_state, d_out);
    const uint32_t es = (uint32_t)end_state;
    VIT_HIP_CHECK(hipMemcpyAsync(d_end_state, &es, 4, hipMemcpyHostToDevice, h->stream));
    return lds_chainback(h, d_rows, 1, L, d_out, d_end_state, h->stream);
}

// One frame's update through the staging pair.  Device scratch and pinned stage share one layout: [metrics | renorm sum | symbols]
// in, [metrics | renorm sum | what the caller appends] out -- ONE copy each way per call (five pageable copies before: this route is
// called once per trellis step by streaming callers, examples/helpers/puncture_code_helpers.h:51)
struct UpdateStage {
    size_t sym_bytes = 0, met_bytes = 0, met_b = 0, sym_b = 0, in_b = 0;    // _b: rounded up to 256; in_b: the whole input part
    static constexpr size_t rs_b = 256;
    uint8_t *base = nullptr, *hs = nullptr;                                  // device scratch (the metrics are its head), pinned stage
    uint64_t* d_rs() const { return (uint64_t*)(base + met_b); }
    uint8_t* d_sym() const { return base + met_b + rs_b; }
};
// lays the buffers out with `extra_bytes` behind the input part and sends metrics and symbols up on the handle's stream
int stage_update_in(vit_hip_handle h, const void* metrics, const void* symbols, size_t n_steps, size_t extra_bytes, UpdateStage& s) {
    s.sym_bytes = n_steps * (size_t)h->R * (size_t)h->soft_bytes;
    s.met_bytes = (size_t)h->N * (size_t)h->error_bytes;
    s.met_b = align_up(s.met_bytes, 256);
    s.sym_b = align_up(s.sym_bytes, 256);
    s.in_b = s.met_b + s.rs_b + s.sym_b;
    const int rc = ensure_scratch_and_stage(h, s.in_b + extra_bytes);
    if (rc != VIT_HIP_OK) return rc;
    s.base = (uint8_t*)h->d_scratch;
    s.hs = (uint8_t*)h->h_stage;
    memcpy(s.hs, metrics, s.met_bytes);
    memcpy(s.hs + s.met_b + s.rs_b, symbols, s.sym_bytes);
    VIT_HIP_CHECK(hipMemcpyAsync(s.base, s.hs, s.met_b + s.rs_b + s.sym_bytes, hipMemcpyHostToDevice, h->stream));
    return VIT_HIP_OK;
}
// after [metrics | renorm sum] came back into the stage and the stream was synchronised
void stage_update_out(const UpdateStage& s, void* metrics_inout, uint64_t* renorm_sum_out) {
    memcpy(metrics_inout, s.hs, s.met_bytes);
    if (renorm_sum_out) memcpy(renorm_sum_out, s.hs + s.met_b, 8);
}
}  // namespace

extern "C" {

int vit_hip_update_host(vit_hip_handle h, void* metrics_inout, const void* symbols, size_t n_steps,
                        uint64_t* decisions_out, uint64_t* renorm_sum_out) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (!metrics_inout) return fail(VIT_HIP_ERR_INVALID_ARG, "metrics_inout is NULL");
    if (renorm_sum_out) *renorm_sum_out = 0;
    if (n_steps == 0) return VIT_HIP_OK;
    if (!symbols || !decisions_out) return fail(VIT_HIP_ERR_INVALID_ARG, "symbols/decisions_out is NULL");
    if (n_steps > 0x7FFFFFF0u) return fail(VIT_HIP_ERR_INVALID_ARG, "n_steps too large");
    VIT_HIP_ON_DEVICE(h->device);
    const size_t dec_bytes = n_steps * (size_t)h->W * 8;
    UpdateStage s;
    int rc = stage_update_in(h, metrics_inout, symbols, n_steps, align_up(dec_bytes, 256), s);
    if (rc != VIT_HIP_OK) return rc;
    uint64_t* d_dec = (uint64_t*)(s.base + s.in_b);
    // streaming state lives on the host between calls: one frame.  K <= 7 (at most 64 states): the one-wavefront latency kernel
    // (kernels_one.hpp: lane == state, metrics in a register, ~100 clocks per step); K = 8, 9 with R <= 4: its wide sibling (two or
    // four states per lane); larger codes, and every code under VIT_HIP_HOST_ROUTE_LDS: the LDS plan on one frame
    const HostFamily family = host_family(h);
    if (family == HOST_WIDE) {
        OneUpdateWideArgs oa{};
        oa.symbols = s.d_sym();
        oa.sym_total_bytes = s.sym_bytes;
        oa.decisions = d_dec;
        oa.metrics_io = s.base;
        oa.renorm_sum = s.d_rs();
        oa.pattern = h->d_pattern;
        oa.K = h->K;
        oa.n_steps = (int)n_steps;
        oa.cfg = h->cfg;
        VIT_HIP_CHECK(one_wide_launch_update(h->K, h->R, h->shift, oa, h->stream));
    } else if (family != HOST_LDS) {
        OneUpdateArgs oa{};
        oa.symbols = s.d_sym();
        oa.sym_total_bytes = s.sym_bytes;
        oa.decisions = d_dec;
        oa.metrics_io = s.base;
        oa.renorm_sum = s.d_rs();
        oa.pattern = h->d_pattern;
        oa.K = h->K;
        oa.n_steps = (int)n_steps;
        oa.cfg = h->cfg;
        if ((h->shift ? one_launch_update<8>(h->R, oa, h->stream) : one_launch_update<0>(h->R, oa, h->stream)) != 0)
            return fail(VIT_HIP_ERR_RUNTIME, "single-frame update launch failed");
    } else {
        rc = lds_update(h, s.d_sym(), n_steps * (size_t)h->R, 1, n_steps, n_steps, 0, d_dec, s.base, false, s.d_rs(), nullptr, h->stream);
        if (rc != VIT_HIP_OK) return rc;
    }
    // out: metrics and renorm sum sit in front of the symbols, the decision rows behind them: copy [metrics | rs] and the rows
    // as one contiguous range when the symbols are short (the common streaming case), else as two
    if (s.sym_b <= 4096) {
        VIT_HIP_CHECK(hipMemcpyAsync(s.hs, s.base, s.in_b + dec_bytes, hipMemcpyDeviceToHost, h->stream));
        VIT_HIP_CHECK(hipStreamSynchronize(h->stream));
        memcpy(decisions_out, s.hs + s.in_b, dec_bytes);
    } else {
        VIT_HIP_CHECK(hipMemcpyAsync(s.hs, s.base, s.met_b + s.rs_b, hipMemcpyDeviceToHost, h->stream));
        VIT_HIP_CHECK(hipMemcpyAsync(s.hs + s.met_b + s.rs_b, d_dec, dec_bytes, hipMemcpyDeviceToHost, h->stream));
        VIT_HIP_CHECK(hipStreamSynchronize(h->stream));
        memcpy(decisions_out, s.hs + s.met_b + s.rs_b, dec_bytes);
    }
    stage_update_out(s, metrics_inout, renorm_sum_out);
    return VIT_HIP_OK;
}

int vit_hip_chainback_host(vit_hip_handle h, const uint64_t* decisions, size_t L, size_t end_state, uint8_t* bytes_out) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (L == 0) return VIT_HIP_OK;
    if (!decisions || !bytes_out) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL buffer");
    if (end_state >= (size_t)h->N) return fail(VIT_HIP_ERR_INVALID_ARG, "end_state out of range");
    VIT_HIP_ON_DEVICE(h->device);
    const size_t rows = L + (size_t)h->K - 1;
    const size_t dec_b = align_up(rows * (size_t)h->W * 8, 256);
    const size_t out_b = align_up((L + 7) / 8, 256);
    // one pinned staging copy each way (pageable copies go through the runtime's own staging and synchronise more often)
    int rc = ensure_scratch_and_stage(h, dec_b + out_b + 256);
    if (rc != VIT_HIP_OK) return rc;
    uint8_t* base = (uint8_t*)h->d_scratch;
    const size_t dec_bytes = rows * (size_t)h->W * 8, out_bytes = (L + 7) / 8;
    uint8_t* hs = (uint8_t*)h->h_stage;
    memcpy(hs, decisions, dec_bytes);
    VIT_HIP_CHECK(hipMemcpyAsync(base, hs, dec_bytes, hipMemcpyHostToDevice, h->stream));
    rc = chainback_one_frame(h, (const uint64_t*)base, L, end_state, base + dec_b, (uint32_t*)(base + dec_b + out_b));
    if (rc != VIT_HIP_OK) return rc;
    VIT_HIP_CHECK(hipMemcpyAsync(hs + dec_b, base + dec_b, out_bytes, hipMemcpyDeviceToHost, h->stream));
    VIT_HIP_CHECK(hipStreamSynchronize(h->stream));
    memcpy(bytes_out, hs + dec_b, out_bytes);
    return VIT_HIP_OK;
}

// ---- frame route: ONE launch for update() + the chainback() that follows, rows kept on the device -----------------------------
int vit_hip_update_host_lazy(vit_hip_handle h, void* metrics_inout, const void* symbols, size_t n_steps, size_t first_row,
                             size_t speculate_bits, size_t speculate_end_state, uint64_t* renorm_sum_out) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (!metrics_inout) return fail(VIT_HIP_ERR_INVALID_ARG, "metrics_inout is NULL");
    if (renorm_sum_out) *renorm_sum_out = 0;
    if (n_steps == 0) return VIT_HIP_OK;
    if (!symbols) return fail(VIT_HIP_ERR_INVALID_ARG, "symbols is NULL");
    if (n_steps > 0x7FFFFFF0u || first_row > 0x7FFFFFF0u) return fail(VIT_HIP_ERR_INVALID_ARG, "n_steps / first_row too large");
    if (speculate_bits > 0 && speculate_end_state >= (size_t)h->N) return fail(VIT_HIP_ERR_INVALID_ARG, "speculate_end_state out of range");
    VIT_HIP_ON_DEVICE(h->device);
    h->spec_valid = false;                                   // whatever was decoded ahead belonged to the rows as they were
    int rc = ensure_rows(h, first_row + n_steps);
    if (rc != VIT_HIP_OK) return rc;
    const size_t sym_bytes = n_steps * (size_t)h->R * (size_t)h->soft_bytes;
    const size_t met_bytes = (size_t)h->N * (size_t)h->error_bytes;
    const HostFamily family = host_family(h);
    if (family == HOST_LDS) {
        // no single-frame kernel (or none wanted): the LDS plan on one frame, as vit_hip_update_host runs it -- but the rows go
        // straight into the device row store
        UpdateStage s;
        rc = stage_update_in(h, metrics_inout, symbols, n_steps, 0, s);
        if (rc != VIT_HIP_OK) return rc;
        rc = lds_update(h, s.d_sym(), n_steps * (size_t)h->R, 1, n_steps, n_steps, 0, h->d_rows + first_row * (size_t)h->W, s.base, false,
                        s.d_rs(), nullptr, h->stream);
        if (rc != VIT_HIP_OK) return rc;
        VIT_HIP_CHECK(hipMemcpyAsync(s.hs, s.base, s.met_b + s.rs_b, hipMemcpyDeviceToHost, h->stream));
        VIT_HIP_CHECK(hipStreamSynchronize(h->stream));
        stage_update_out(s, metrics_inout, renorm_sum_out);
        return VIT_HIP_OK;
    }
    const bool spec = speculate_bits > 0 && first_row + n_steps == speculate_bits + (size_t)h->K - 1 && speculate_bits <= 0xFFFFFFF0ull;
    const size_t met_off = 256, sym_off = met_off + align_up(met_bytes, 256), out_off = sym_off + align_up(sym_bytes, 256);
    const size_t out_bytes = spec ? (speculate_bits + 7) / 8 : 0;
    rc = ensure_map(h, out_off + align_up(out_bytes, 256));
    if (rc != VIT_HIP_OK) return rc;
    uint8_t* hm = (uint8_t*)h->h_map;
    void* dm_v = nullptr;
    VIT_HIP_CHECK(hipHostGetDevicePointer(&dm_v, h->h_map, 0));
    uint8_t* dm = (uint8_t*)dm_v;
    memcpy(hm + sym_off, symbols, sym_bytes);
    const uint32_t seq = ++h->seq ? h->seq : ++h->seq;       // never 0
    // OneFrameArgs and OneFrameWideArgs differ in the number of start metrics they carry (64 / 256)
    auto fill = [&](auto& fa) {
        fa.u.symbols = dm + sym_off;
        fa.u.sym_total_bytes = sym_bytes;
        fa.u.decisions = h->d_rows + first_row * (size_t)h->W;
        fa.u.metrics_io = dm + met_off;
        fa.u.renorm_sum = (uint64_t*)(dm + 64);
        fa.u.pattern = h->d_pattern;
        fa.u.K = h->K;
        fa.u.n_steps = (int)n_steps;
        fa.u.cfg = h->cfg;
        fa.u.metrics_in_args = 1;
        for (int s = 0; s < (int)(sizeof(fa.u.metrics_in) / sizeof(fa.u.metrics_in[0])); ++s) {
            const int t = s & (h->N - 1);
            fa.u.metrics_in[s] = h->error_bytes == 1 ? (uint16_t)((uint32_t)((const uint8_t*)metrics_inout)[t] << 8) : ((const uint16_t*)metrics_inout)[t];
        }
        fa.do_chainback = spec ? 1 : 0;
        fa.c.decisions = h->d_rows;
        fa.c.out = dm + out_off;
        fa.c.end_state = (uint32_t)speculate_end_state;
        fa.c.L = (uint32_t)speculate_bits;
        fa.c.K = h->K;
        fa.seq = seq;
        fa.done = (uint32_t*)dm;
    };
    volatile uint32_t* done = (volatile uint32_t*)hm;
    int launched;
    if (family == HOST_WIDE) {
        OneFrameWideArgs fa{};
        fill(fa);
        launched = one_wide_launch_frame(h->K, h->R, h->shift, fa, h->stream) == hipSuccess ? 0 : -1;
    } else {
        OneFrameArgs fa{};
        fill(fa);
        launched = h->shift ? one_launch_frame<8>(h->R, fa, h->stream) : one_launch_frame<0>(h->R, fa, h->stream);
    }
    if (launched != 0) return fail(VIT_HIP_ERR_RUNTIME, "frame kernel launch failed");
    // the kernel's last act is a system-scope release store of seq into the control word: poll it (a stream synchronisation costs more
    // than the whole chainback); a kernel that never gets there shows up in the stream's status
    for (uint64_t spins = 0; __atomic_load_n(done, __ATOMIC_ACQUIRE) != seq; ++spins) {
        if ((spins & 0xFFFFu) == 0xFFFFu) {
            const hipError_t q = hipStreamQuery(h->stream);
            if (q != hipErrorNotReady) {
                if (q != hipSuccess) return fail(VIT_HIP_ERR_RUNTIME, std::string("frame kernel: ") + hipGetErrorString(q));
                if (__atomic_load_n(done, __ATOMIC_ACQUIRE) != seq) return fail(VIT_HIP_ERR_RUNTIME, "frame kernel finished without reporting");
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    // let the runtime see that the launch has retired: polled completions never pass through it, and a queue it believes full of
    // pending kernels is drained the hard way once in ~200 launches (two 38 ms calls in 400)
    (void)hipStreamQuery(h->stream);
    memcpy(metrics_inout, hm + met_off, met_bytes);
    if (renorm_sum_out) memcpy(renorm_sum_out, hm + 64, 8);
    if (spec) { h->spec_valid = true; h->spec_bits = speculate_bits; h->spec_end = speculate_end_state; h->spec_off = out_off; }
    return VIT_HIP_OK;
}

int vit_hip_fetch_decisions_host(vit_hip_handle h, size_t first_row, size_t n_rows, uint64_t* decisions_out) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (n_rows == 0) return VIT_HIP_OK;
    if (!decisions_out) return fail(VIT_HIP_ERR_INVALID_ARG, "decisions_out is NULL");
    if (first_row + n_rows > h->rows_cap || !h->d_rows) return fail(VIT_HIP_ERR_INVALID_ARG, "rows outside the device row store");
    VIT_HIP_ON_DEVICE(h->device);
    VIT_HIP_CHECK(hipMemcpyAsync(decisions_out, h->d_rows + first_row * (size_t)h->W, n_rows * (size_t)h->W * 8, hipMemcpyDeviceToHost, h->stream));
    VIT_HIP_CHECK(hipStreamSynchronize(h->stream));
    return VIT_HIP_OK;
}

int vit_hip_chainback_host_lazy(vit_hip_handle h, size_t L, size_t end_state, uint8_t* bytes_out) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (L == 0) return VIT_HIP_OK;
    if (!bytes_out) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL buffer");
    if (end_state >= (size_t)h->N) return fail(VIT_HIP_ERR_INVALID_ARG, "end_state out of range");
    const size_t rows = L + (size_t)h->K - 1, out_bytes = (L + 7) / 8;
    if (rows > h->rows_cap || !h->d_rows) return fail(VIT_HIP_ERR_INVALID_ARG, "the device row store does not hold L + K - 1 rows");
    if (h->spec_valid && h->spec_bits == L && h->spec_end == end_state) {      // decoded by the launch that completed the frame
        memcpy(bytes_out, (const uint8_t*)h->h_map + h->spec_off, out_bytes);
        return VIT_HIP_OK;
    }
    VIT_HIP_ON_DEVICE(h->device);
    const size_t out_b = align_up(out_bytes, 256);
    int rc = ensure_scratch_and_stage(h, out_b + 256);
    if (rc != VIT_HIP_OK) return rc;
    uint8_t* base = (uint8_t*)h->d_scratch;
    rc = chainback_one_frame(h, h->d_rows, L, end_state, base, (uint32_t*)(base + out_b));
    if (rc != VIT_HIP_OK) return rc;
    VIT_HIP_CHECK(hipMemcpyAsync(h->h_stage, base, out_bytes, hipMemcpyDeviceToHost, h->stream));
    VIT_HIP_CHECK(hipStreamSynchronize(h->stream));
    memcpy(bytes_out, h->h_stage, out_bytes);
    return VIT_HIP_OK;
}

const char* vit_hip_host_route_note(vit_hip_handle h) {
    if (!h) return "NULL handle";
    thread_local std::string note;
    char head[48];
    snprintf(head, sizeof(head), "K=%d R=%d: ", h->K, h->R);
    note = head;
    switch (host_family(h)) {
        case HOST_ONE7:
            note += "single-frame in-place (K = 7): one wavefront walks the trellis in place, two helper wavefronts make its branch metrics "
                    "and its decision rows (csrc/kernels_one.hpp: one_update7_kernel, one_frame7_kernel)";
            break;
        case HOST_ONE:
            note += "single-frame lane == state: one wavefront, one state per lane (csrc/kernels_one.hpp: one_update_kernel, one_frame_kernel)";
            break;
        case HOST_WIDE:
            note += "single-frame wide (K = 8, 9): one wavefront, lane == state mod 64, " + std::to_string(h->N / 64) +
                    " states per lane (csrc/kernels_one.hpp: one_update_wide_kernel, one_frame_wide_kernel)";
            break;
        default:
            note += "PLAN_LDS on one frame (the general LDS kernels: two workgroup barriers per trellis step)";
            if (h->host_route == VIT_HIP_HOST_ROUTE_LDS) note += "; forced by vit_hip_set_host_route(h, VIT_HIP_HOST_ROUTE_LDS)";
            else if (h->K >= 10) note += "; the single-frame kernels serve K <= 9: K >= 10";
            else note += "; the single-frame kernels serve R <= 4 at K = 8, 9: R >= 5";
    }
    return note.c_str();
}

int vit_hip_set_host_route(vit_hip_handle h, int route) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (route != VIT_HIP_HOST_ROUTE_AUTO && route != VIT_HIP_HOST_ROUTE_LDS)
        return fail(VIT_HIP_ERR_INVALID_ARG, "route must be VIT_HIP_HOST_ROUTE_AUTO or VIT_HIP_HOST_ROUTE_LDS");
    h->host_route = route;
    return VIT_HIP_OK;
}

}  // extern "C"
