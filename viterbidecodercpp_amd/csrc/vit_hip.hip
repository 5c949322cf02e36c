// vit_hip.hip -- C ABI (include/vit_hip.h) over the gfx950 kernels: the decoder handle, plan selection, workspace layout and the
// batched entry points.  Host-side logic only: argument checking and launches.  There is no CPU decode path in this library:
// without a usable GPU every entry point fails with VIT_HIP_ERR_NO_DEVICE / VIT_HIP_ERR_RUNTIME.  The other routes of the ABI
// live in vit_windows.hip, vit_pipeline.hip, vit_host.hip, vit_tools.hip and vit_encode.hip (vit_internal.hpp says what they share).
#include <stdio.h>

#include "vit_internal.hpp"
#include "kernels_lds.hpp"
#include "kernels_lds2.hpp"
#include "kernels_depuncture.hpp"
#include "reg_jit.hpp"

using namespace vit;

namespace vit {
// ViterbiDecoder_Core::reset (core.h:202-211) for a batch: metrics [F][N] error_t
template <typename error_t>
__global__ void reset_kernel(error_t* met, const uint32_t* start, size_t frames, uint32_t N, uint32_t init_start, uint32_t init_non_start) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= frames * N) return;
    const size_t f = idx / N;
    const uint32_t s = (uint32_t)(idx % N);
    const uint32_t st = start ? (start[f] & (N - 1u)) : 0u;
    met[idx] = (error_t)(s == st ? init_start : init_non_start);
}

}  // namespace vit

namespace {
int lds_waves(int N) {
    if (N <= 256) return 1;
    int w = N / 256;
    return w > 16 ? 16 : w;
}

size_t lds_smem_bytes(int N, int waves) {
    const int H = N / 2;
    const int pat = N <= 16384 ? (H > 0 ? H : 1) : 0;     // K = 16 reads the patterns from global memory (kernels_lds.hpp)
    return (size_t)(2 * N + pat + waves) * sizeof(uint16_t);
}

// run-time compiled PLAN_REG for polynomials outside the ahead-of-time table (reg_jit.hpp)
// package_only: load an install-time precompiled code object if the package cache holds one; compile nothing
bool try_reg_jit(vit_hip_handle h, bool package_only) {
    // (a handle on the GENERIC kernels asks again when the caller allows compiling: kernels specialised for its polynomials are faster)
    if (h->reg_ok && !(h->reg_code.generic && !package_only)) return true;
    if (!h->linear || !vit::reg_jit_supported(h->K, h->R)) return false;
    std::string err;
    const vit::RegJitModule* m = vit::reg_jit_get(h->K, h->R, h->G, h->shift, h->device, package_only, err, &h->reg_origin);
    bool generic = false;
    if (!m && vit::reg_generic_supported(h->K, h->R)) {
        // no kernels specialised for these polynomials (and, unless package_only, no compiler to make them): the GENERIC code object
        // of this (K, R) -- polynomials read from the kernel arguments (RegSpec::GENERIC) -- if the package cache holds it
        const uint32_t zero[6] = {0, 0, 0, 0, 0, 0};
        std::string err2;
        m = vit::reg_jit_get(h->K, h->R, zero, h->shift, h->device, true, err2, &h->reg_origin);
        generic = m != nullptr;
    }
    if (!m) {
        if (h->reg_ok) return true;             // the upgrade failed: the generic kernels stay
        if (!package_only) last_error() = err;
        return false;
    }
    h->reg_code.id = -1;
    h->reg_code.K = h->K;
    h->reg_code.R = h->R;
    h->reg_code.tile = reg_tile_frames(h->K);
    h->reg_code.jit = m;
    h->reg_code.generic = generic;
    for (int i = 0; i < 6; ++i) h->reg_code.G[i] = i < h->R ? h->G[i] : 0u;
    h->reg_ok = true;
    return true;
}

int read_soft(const void* p, size_t idx, int soft_bytes) {
    return soft_bytes == 1 ? (int)((const int8_t*)p)[idx] : (int)((const int16_t*)p)[idx];
}

unsigned parity_u32(uint32_t x) { return (unsigned)__builtin_popcount(x) & 1u; }

template <int R, int SHIFT>
int launch_lds_update_t(const vit::LdsUpdateArgs& a, size_t frames, int N, hipStream_t st) {
    const int waves = lds_waves(N);
    const size_t smem = lds_smem_bytes(N, waves);
    auto kern = vit::lds_update_kernel<R, SHIFT>;
    if (smem > 64 * 1024) {
        VIT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)smem));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)frames), dim3(64 * waves), smem, st, a);
    VIT_HIP_CHECK(hipGetLastError());
    return VIT_HIP_OK;
}

}  // namespace

namespace vit {
int lds_update(vit_hip_handle h, const void* d_symbols, size_t sym_stride, size_t frames, size_t n_steps, size_t rows,
               uint32_t row0, uint64_t* d_decisions, void* d_metrics, bool reset, uint64_t* d_renorm, const uint32_t* d_start,
               hipStream_t st) {
    if (frames == 0 || n_steps == 0) return VIT_HIP_OK;
    vit::LdsUpdateArgs a{};
    a.symbols = (const uint8_t*)d_symbols;
    a.sym_frame_stride_bytes = sym_stride * (size_t)h->soft_bytes;
    a.sym_total_bytes = (frames - 1) * a.sym_frame_stride_bytes + n_steps * (size_t)h->R * (size_t)h->soft_bytes;
    a.decisions = d_decisions;
    a.dec_frame_stride_words = rows * (size_t)h->W;
    a.dec_row0 = row0;
    a.metrics_io = d_metrics;
    a.renorm_sum = d_renorm;
    a.start_state = d_start;
    a.pattern = h->d_pattern;
    a.K = h->K;
    a.n_steps = (int)n_steps;
    a.reset = reset ? 1 : 0;
    a.cfg = h->cfg;
    const int rc = with_rate(h->R, 1, [&](auto r) {
        return h->shift ? launch_lds_update_t<r(), 8>(a, frames, h->N, st) : launch_lds_update_t<r(), 0>(a, frames, h->N, st);
    });
    return rc == 1 ? fail(VIT_HIP_ERR_UNSUPPORTED, "code rate R must be 1..8") : rc;
}

int lds_chainback(vit_hip_handle h, const uint64_t* d_decisions, size_t frames, size_t L, uint8_t* d_out,
                  const uint32_t* d_end, hipStream_t st) {
    if (frames == 0 || L == 0) return VIT_HIP_OK;
    vit::LdsChainbackArgs a{};
    a.decisions = d_decisions;
    a.dec_frame_stride_words = (L + (size_t)h->K - 1) * (size_t)h->W;
    a.out = d_out;
    a.end_state = d_end;
    a.frames = frames;
    a.L = L;
    a.K = h->K;
    const int block = 64;
    hipLaunchKernelGGL(vit::lds_chainback_kernel, dim3((unsigned)((frames + block - 1) / block)), dim3(block), 0, st, a);
    VIT_HIP_CHECK(hipGetLastError());
    return VIT_HIP_OK;
}

bool lds2_chainback_fits(vit_hip_handle h) { return lds2_chainback_fits_beside_update(h->K, h->R, h->shift); }
}  // namespace vit

extern "C" {

const char* vit_hip_last_error(void) { return last_error().c_str(); }

int vit_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int vit_hip_create_impl(int K, int R, int soft_bytes, int error_bytes, const void* branch_table, const void* config,
                   int device, vit_hip_handle* out) {
    if (!out) return fail(VIT_HIP_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!branch_table || !config) return fail(VIT_HIP_ERR_INVALID_ARG, "branch_table/config is NULL");
    if (K < 2 || K > 16) return fail(VIT_HIP_ERR_UNSUPPORTED, "constraint length K must be 2..16 (the 2^(K-1) state metrics of a frame pair live in one CU's LDS)");
    if (R < 1 || R > 8) return fail(VIT_HIP_ERR_UNSUPPORTED, "code rate R must be 1..8");
    if (!((soft_bytes == 2 && error_bytes == 2) || (soft_bytes == 1 && error_bytes == 1)))
        return fail(VIT_HIP_ERR_UNSUPPORTED, "(soft_t,error_t) must be (int16_t,uint16_t) or (int8_t,uint8_t)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(VIT_HIP_ERR_NO_DEVICE, "no HIP device available (this library has no CPU decode path)");
    if (device < 0 || device >= ndev) return fail(VIT_HIP_ERR_INVALID_ARG, "device index out of range");

    vit_hip_decoder* h = new vit_hip_decoder();
    h->K = K; h->R = R; h->soft_bytes = soft_bytes; h->error_bytes = error_bytes; h->device = device;
    h->N = 1 << (K - 1); h->H = h->N / 2; h->W = h->N >= 64 ? h->N / 64 : 1;
    h->shift = soft_bytes == 1 ? 8 : 0;
    const int Ht = h->H > 0 ? h->H : 1;   // K=2 still stores one half-state

    // the table is two-valued: low == value at half-state 0 (parity of 0 is 0), high == the other value
    const int low = read_soft(branch_table, 0, soft_bytes);
    int high = low;
    bool have_high = false;
    for (int i = 0; i < R; ++i)
        for (int s = 0; s < Ht; ++s) {
            const int v = read_soft(branch_table, (size_t)i * Ht + s, soft_bytes);
            if (v != low) {
                if (!have_high) { high = v; have_high = true; }
                else if (v != high) { delete h; return fail(VIT_HIP_ERR_INVALID_ARG, "branch table holds more than two distinct values"); }
            }
        }
    for (int i = 0; i < R; ++i)
        if (read_soft(branch_table, (size_t)i * Ht, soft_bytes) != low) {
            delete h;
            return fail(VIT_HIP_ERR_INVALID_ARG, "branch table row does not start with the low value");
        }
    if (!have_high) high = low;  // degenerate code: every expected symbol is `low`
    h->high = high; h->low = low;
    h->pattern.assign(Ht, 0);
    for (int i = 0; i < R; ++i)
        for (int s = 0; s < Ht; ++s)
            if (have_high && read_soft(branch_table, (size_t)i * Ht + s, soft_bytes) == high) h->pattern[s] |= (uint16_t)(1u << i);

    // recover the polynomials (middle bits from the unit half-states; bit 0 and bit K-1 are implied by the butterfly
    // identity the reference relies on, viterbi_decoder_scalar.h:85-95) and check that the table is linear
    for (int i = 0; i < R; ++i) {
        uint32_t g = 1u | (1u << (K - 1));
        for (int k = 0; k + 2 < K; ++k)
            if ((h->pattern[(size_t)1 << k] >> i) & 1u) g |= 1u << (k + 1);
        h->G[i] = g;
    }
    h->linear = true;
    for (int s = 0; s < Ht && h->linear; ++s)
        for (int i = 0; i < R; ++i)
            if (parity_u32(((uint32_t)s << 1) & h->G[i] & ~(1u | (1u << (K - 1)))) != ((h->pattern[s] >> i) & 1u)) { h->linear = false; break; }

    for (int k = 0; k < 4; ++k)
        h->cfg_raw[k] = error_bytes == 1 ? (uint32_t)((const uint8_t*)config)[k] : (uint32_t)((const uint16_t*)config)[k];
    // a table that never shows a second value (K = 2 always: one half-state per polynomial, and that one reads low) cannot say what
    // `high` is, and the encoder, the frame generator and the symbol counts would take it for `low`: soft_decision_max_error =
    // (high - low) R says it.  Only h->high, which those read; the decode kernels keep the values the table gave them (cfg.high below)
    if (!have_high && h->cfg_raw[0] > 0 && h->cfg_raw[0] % (uint32_t)R == 0 &&
        low + (int)(h->cfg_raw[0] / (uint32_t)R) <= (soft_bytes == 2 ? 32767 : 127))
        h->high = low + (int)(h->cfg_raw[0] / (uint32_t)R);
    h->cfg.max_error = (uint16_t)(h->cfg_raw[0] << h->shift);
    h->cfg.init_start = (uint16_t)(h->cfg_raw[1] << h->shift);
    h->cfg.init_non_start = (uint16_t)(h->cfg_raw[2] << h->shift);
    h->cfg.threshold = (uint16_t)(h->cfg_raw[3] << h->shift);
    h->cfg.high = (int16_t)(uint16_t)((uint32_t)high << h->shift);
    h->cfg.low = (int16_t)(uint16_t)((uint32_t)low << h->shift);

    DeviceGuard guard(device);
    if (!guard.ok) { delete h; return fail(VIT_HIP_ERR_RUNTIME, "hipSetDevice failed"); }
    if (hipMalloc((void**)&h->d_pattern, Ht * sizeof(uint16_t)) != hipSuccess ||
        hipMemcpy(h->d_pattern, h->pattern.data(), Ht * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        if (h->d_pattern) (void)hipFree(h->d_pattern);
        delete h;
        return fail(VIT_HIP_ERR_RUNTIME, "device allocation failed in vit_hip_create");
    }
    h->reg_ok = h->linear && vit::reg_code_supported(K, R) && vit::reg_code_init(&h->reg_code, K, R, h->G, h->cfg);
    if (!h->reg_ok && h->linear && vit::reg_jit_supported(K, R)) {
        // a code object precompiled at install time (package cache, reg_jit.hpp) is as good as a built-in one: no compiler runs
        const char* e = getenv("VIT_HIP_JIT");
        // compiling: opt-in at create time (vit_hip_set_plan(PLAN_REG) always tries); either way the search ends at the package's GENERIC kernels
        if (e && *e == '1') (void)try_reg_jit(h, false);
        else (void)try_reg_jit(h, true);
    }
    h->lds2_ok = h->linear && vit::lds2_supported(K, R);   // the group-B tables rely on the code being linear
    h->plan = h->reg_ok ? VIT_HIP_PLAN_REG : h->lds2_ok ? VIT_HIP_PLAN_LDS2 : VIT_HIP_PLAN_LDS;
    *out = h;
    return VIT_HIP_OK;
}

int vit_hip_create(int K, int R, int soft_bytes, int error_bytes, const void* branch_table, const void* config,
                   int device, vit_hip_handle* out) {
    VIT_HIP_NOTHROW(return vit_hip_create_impl(K, R, soft_bytes, error_bytes, branch_table, config, device, out));
}

int vit_hip_destroy(vit_hip_handle h) {
    if (!h) return VIT_HIP_OK;
    DeviceGuard guard(h->device);
    if (h->d_pattern) (void)hipFree(h->d_pattern);
    if (h->d_scratch) (void)hipFree(h->d_scratch);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->h_map) (void)hipHostFree(h->h_map);
    if (h->d_rows) (void)hipFree(h->d_rows);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return VIT_HIP_OK;
}

const char* vit_hip_plan_note(vit_hip_handle h) {
    if (!h) return "NULL handle";
    thread_local std::string note;
    char head[160];
    snprintf(head, sizeof(head), "K=%d R=%d: %s", h->K, h->R,
             h->plan == VIT_HIP_PLAN_REG ? "PLAN_REG (state metrics in registers, 32-128 frames per wavefront)"
             : h->plan == VIT_HIP_PLAN_LDS2 ? "PLAN_LDS2 (frame pair per workgroup, four trellis steps per barrier)"
                                            : "PLAN_LDS, the COMPATIBILITY plan (one frame per workgroup: ~20x slower per state update than the other plans)");
    note = head;
    if (h->plan == VIT_HIP_PLAN_REG && h->reg_code.jit) {
        const bool pkg = h->reg_origin.compare(0, vit::package_cache_dir().size(), vit::package_cache_dir()) == 0;
        note += std::string(pkg ? "; kernels precompiled at install time, loaded from the package cache " : "; kernels compiled at run time, loaded from the user cache ") + h->reg_origin;
        if (h->reg_code.generic)
            note += "; these are the GENERIC kernels of this (K, R) -- polynomials read at run time, 2 - 20 % behind kernels specialised for them: "
                    "python -m viterbidecodercpp_amd.tools.precompile K R G... at install time, or VIT_HIP_JIT=1 before vit_hip_create (hipcc), gets those";
    }
    if (h->plan == VIT_HIP_PLAN_LDS) {
        if (h->reg_ok || (h->linear && vit::reg_jit_supported(h->K, h->R)))
            note += h->reg_ok ? "; the register plan is available: vit_hip_set_plan(h, VIT_HIP_PLAN_REG)"
                              : "; a register-plan instantiation for these polynomials can be compiled at run time: vit_hip_set_plan(h, VIT_HIP_PLAN_REG) "
                                "(hipcc, 30-60 s once, cached on disk), or VIT_HIP_JIT=1 before vit_hip_create; or at install time, for hosts without a "
                                "compiler: python -m viterbidecodercpp_amd.tools.precompile K R G... (vit_hip_precompile)";
        else if (h->lds2_ok)
            note += "; PLAN_LDS2 is available: vit_hip_set_plan(h, VIT_HIP_PLAN_LDS2)";
        else if (!h->linear)
            note += "; no faster plan: the branch table is not that of a linear convolutional code";
        else
            note += "; no faster plan exists for this (K, R): the register plan serves K = 2..9 with R <= 6, PLAN_LDS2 K = 10..16 with R <= 6";
    }
    return note.c_str();
}

int vit_hip_get_info(vit_hip_handle h, vit_hip_info* info) {
    if (!h || !info) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL argument");
    memset(info, 0, sizeof(*info));
    info->K = h->K; info->R = h->R; info->soft_bytes = h->soft_bytes; info->error_bytes = h->error_bytes;
    info->num_states = h->N; info->decision_words = h->W; info->device = h->device; info->plan = h->plan;
    info->soft_decision_high = h->high; info->soft_decision_low = h->low;
    for (int i = 0; i < h->R && i < 16; ++i) info->polynomials[i] = h->linear ? h->G[i] : 0u;
    info->table_is_linear = h->linear ? 1 : 0;
    info->workspace_tile_frames = h->plan == VIT_HIP_PLAN_REG ? h->reg_code.tile : h->plan == VIT_HIP_PLAN_LDS2 ? 2 : 1;
    return VIT_HIP_OK;
}

static int vit_hip_set_plan_impl(vit_hip_handle h, int plan) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (plan == VIT_HIP_PLAN_AUTO) plan = h->reg_ok ? VIT_HIP_PLAN_REG : h->lds2_ok ? VIT_HIP_PLAN_LDS2 : VIT_HIP_PLAN_LDS;
    // (a handle on the package's GENERIC kernels: asking for the register plan by name looks for kernels specialised for its polynomials --
    // package cache, user cache, compiler -- and keeps the generic ones when there are none)
    if (plan == VIT_HIP_PLAN_REG && (!h->reg_ok || (h->reg_code.jit && h->reg_code.generic))) {
        DeviceGuard guard(h->device);
        last_error().clear();
        if (!guard.ok || !try_reg_jit(h, false))
            return fail(VIT_HIP_ERR_UNSUPPORTED, "PLAN_REG not available for this code: " +
                        (last_error().empty() ? std::string("K must be 2..9 and R <= 6, linear branch table") : std::string(last_error())));
    }
    if (plan == VIT_HIP_PLAN_LDS2 && !h->lds2_ok)
        return fail(VIT_HIP_ERR_UNSUPPORTED, "PLAN_LDS2 serves K = 10..16 with R <= 6 and a linear branch table (see kernels_lds2.hpp)");
    if (plan != VIT_HIP_PLAN_LDS && plan != VIT_HIP_PLAN_REG && plan != VIT_HIP_PLAN_LDS2)
        return fail(VIT_HIP_ERR_INVALID_ARG, "unknown plan");
    h->plan = plan;
    return VIT_HIP_OK;
}

int vit_hip_set_plan(vit_hip_handle h, int plan) { VIT_HIP_NOTHROW(return vit_hip_set_plan_impl(h, plan)); }

size_t vit_hip_blob_bytes(int K, int R, int soft_bytes, int error_bytes) {
    if (K < 2 || K > 30 || R < 1 || R > 64 || soft_bytes < 1 || soft_bytes > 8 || error_bytes < 1 || error_bytes > 8) return 0;
    const size_t Ht = K > 2 ? ((size_t)1 << (K - 2)) : 1;
    return sizeof(BlobHeader) + (size_t)R * Ht * (size_t)soft_bytes + 4 * (size_t)error_bytes;
}

int vit_hip_pack_blob(int K, int R, int soft_bytes, int error_bytes, const void* branch_table, const void* config,
                      void* blob, size_t blob_bytes) {
    const size_t need = vit_hip_blob_bytes(K, R, soft_bytes, error_bytes);
    if (!need || !branch_table || !config || !blob) return fail(VIT_HIP_ERR_INVALID_ARG, "bad blob arguments");
    if (blob_bytes < need) return fail(VIT_HIP_ERR_INVALID_ARG, "blob buffer too small");
    BlobHeader hd{BLOB_MAGIC, K, R, soft_bytes, error_bytes};
    uint8_t* p = (uint8_t*)blob;
    memcpy(p, &hd, sizeof(hd));
    const size_t tb = need - sizeof(hd) - 4 * (size_t)error_bytes;
    memcpy(p + sizeof(hd), branch_table, tb);
    memcpy(p + sizeof(hd) + tb, config, 4 * (size_t)error_bytes);
    return VIT_HIP_OK;
}

static int vit_hip_create_from_blob_impl(const void* blob, size_t blob_bytes, int device, vit_hip_handle* out) {
    if (!blob || blob_bytes < sizeof(BlobHeader)) return fail(VIT_HIP_ERR_INVALID_ARG, "blob too small");
    BlobHeader hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != BLOB_MAGIC) return fail(VIT_HIP_ERR_INVALID_ARG, "bad blob magic");
    // the header is untrusted: validate before any size arithmetic
    if (hd.K < 2 || hd.K > 16 || hd.R < 1 || hd.R > 8 ||
        !((hd.soft_bytes == 2 && hd.error_bytes == 2) || (hd.soft_bytes == 1 && hd.error_bytes == 1)))
        return fail(VIT_HIP_ERR_INVALID_ARG, "corrupt blob header");
    const size_t need = vit_hip_blob_bytes(hd.K, hd.R, hd.soft_bytes, hd.error_bytes);
    if (!need || blob_bytes < need) return fail(VIT_HIP_ERR_INVALID_ARG, "blob truncated");
    const uint8_t* p = (const uint8_t*)blob + sizeof(hd);
    const size_t tb = need - sizeof(hd) - 4 * (size_t)hd.error_bytes;
    // copies keep the caller free of alignment requirements
    std::vector<uint16_t> table((tb + 1) / 2), cfg(4);
    memcpy(table.data(), p, tb);
    memcpy(cfg.data(), p + tb, 4 * (size_t)hd.error_bytes);
    return vit_hip_create(hd.K, hd.R, hd.soft_bytes, hd.error_bytes, table.data(), cfg.data(), device, out);
}

int vit_hip_create_from_blob(const void* blob, size_t blob_bytes, int device, vit_hip_handle* out) {
    VIT_HIP_NOTHROW(return vit_hip_create_from_blob_impl(blob, blob_bytes, device, out));
}

size_t vit_hip_workspace_bytes(vit_hip_handle h, size_t frames, size_t L) {
    if (!h) return 0;
    switch (h->plan) {
        case VIT_HIP_PLAN_REG: return reg_workspace_bytes(h->reg_code, frames, L);
        case VIT_HIP_PLAN_LDS2: return align_up(lds2_workspace_bytes(h->K, frames, L), 256);
        default: return align_up(frames * (L + (size_t)h->K - 1) * (size_t)h->W * 8, 256);
    }
}

size_t vit_hip_workspace_slab_bytes(vit_hip_handle h, size_t L) {
    if (!h) return 0;
    // PLAN_REG: one tile of frames; PLAN_LDS2: one frame pair (rows x T dwords, T >= 64: a multiple of 256 bytes); PLAN_LDS:
    // the reference layout [F][S][W], dense -- one frame's rows, NOT rounded up to the 256 bytes the whole workspace is
    switch (h->plan) {
        case VIT_HIP_PLAN_REG: return reg_workspace_bytes(h->reg_code, (size_t)h->reg_code.tile, L);
        case VIT_HIP_PLAN_LDS2: return lds2_workspace_bytes(h->K, 2, L);
        default: return (L + (size_t)h->K - 1) * (size_t)h->W * 8;
    }
}

}  // extern "C"

namespace {
// what a launcher of the register plan or of PLAN_LDS2 answered (0, or -1 / -2), as the ABI's result: the one place that words it
int launched(vit_hip_handle h, int rc, const char* what) {
    if (rc == 0) return VIT_HIP_OK;
    return fail(VIT_HIP_ERR_RUNTIME, std::string(h->plan == VIT_HIP_PLAN_REG ? "register-plan " : "PLAN_LDS2 ") + what +
                                         (rc == -2 ? ": a tile's symbols exceed 32-bit offsets" : " launch failed"));
}
}  // namespace

int vit::update_batch_impl(vit_hip_handle h, const void* d_symbols, size_t sym_stride, size_t frames, size_t first_step, size_t n_steps,
                           size_t L, void* d_workspace, size_t workspace_bytes, const void* d_metrics_in, void* d_metrics_out,
                           uint64_t* d_renorm_sum, const uint32_t* d_start_state, vit_hip_stream_t stream, bool overlapped_chunks) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (frames == 0) return VIT_HIP_OK;
    if (!d_symbols || !d_workspace) return fail(VIT_HIP_ERR_INVALID_ARG, "d_symbols/d_workspace is NULL");
    if (first_step + n_steps > L + (size_t)h->K - 1) return fail(VIT_HIP_ERR_INVALID_ARG, "steps exceed traceback length + K-1");
    if (n_steps > 0x7FFFFFF0u || frames > 0x7FFFFFF0u) return fail(VIT_HIP_ERR_INVALID_ARG, "batch too large");
    if (sym_stride == 0) sym_stride = n_steps * (size_t)h->R;
    // the windows of one stream overlap (vit_hip_decode_stream: the kernels only read the symbols); every other caller's chunks do not
    if (sym_stride < n_steps * (size_t)h->R && !overlapped_chunks) return fail(VIT_HIP_ERR_INVALID_ARG, "symbol_frame_stride shorter than one chunk");
    if (workspace_bytes < vit_hip_workspace_bytes(h, frames, L)) return fail(VIT_HIP_ERR_WORKSPACE, "workspace too small");
    if (misaligned(d_workspace, 256)) return fail(VIT_HIP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    if (h->soft_bytes == 2 && misaligned(d_symbols, 2)) return fail(VIT_HIP_ERR_INVALID_ARG, "int16 symbols must be 2-byte aligned");
    if (n_steps == 0) return VIT_HIP_OK;
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    switch (h->plan) {
        case VIT_HIP_PLAN_REG:
            return launched(h, reg_update(h->reg_code, h->cfg, h->shift, d_symbols, sym_stride, frames, first_step, n_steps, L, d_workspace,
                                          d_metrics_in, d_metrics_out, d_renorm_sum, d_start_state, st), "update");
        case VIT_HIP_PLAN_LDS2:
            return launched(h, lds2_update(h->K, h->R, h->cfg, h->shift, h->d_pattern, h->pattern.data(), d_symbols, sym_stride, frames,
                                           first_step, n_steps, L, d_workspace, d_metrics_in, d_metrics_out, d_renorm_sum, d_start_state, st), "update");
        default:
            // PLAN_LDS reads and writes its metrics through one buffer
            if (d_metrics_in && d_metrics_in != d_metrics_out) return fail(VIT_HIP_ERR_INVALID_ARG, "PLAN_LDS resumes in place");
            return lds_update(h, d_symbols, sym_stride, frames, n_steps, L + (size_t)h->K - 1, (uint32_t)first_step, (uint64_t*)d_workspace,
                              d_metrics_out, d_metrics_in == nullptr, d_renorm_sum, d_start_state, st);
    }
}

int vit::chainback_batch_impl(vit_hip_handle h, const void* d_workspace, size_t frames, size_t L, uint8_t* d_bytes_out,
                              const uint32_t* d_end_state, vit_hip_stream_t stream, unsigned wave_priority, bool alt_kernel) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (frames == 0 || L == 0) return VIT_HIP_OK;
    if (!d_workspace || !d_bytes_out) return fail(VIT_HIP_ERR_INVALID_ARG, "d_workspace/d_bytes_out is NULL");
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    switch (h->plan) {
        case VIT_HIP_PLAN_REG:
            return launched(h, reg_chainback(h->reg_code, d_workspace, frames, L, d_bytes_out, d_end_state, st, wave_priority, alt_kernel), "chainback");
        case VIT_HIP_PLAN_LDS2: return launched(h, lds2_chainback(h->K, d_workspace, frames, L, d_bytes_out, d_end_state, st), "chainback");
        default: return lds_chainback(h, (const uint64_t*)d_workspace, frames, L, d_bytes_out, d_end_state, st);
    }
}

extern "C" {

int vit_hip_update_batch(vit_hip_handle h, const void* d_symbols, size_t frames, size_t n_steps, size_t L,
                         void* d_workspace, size_t workspace_bytes, void* d_final_metrics, uint64_t* d_renorm_sum,
                         const uint32_t* d_start_state, vit_hip_stream_t stream) {
    return update_batch_impl(h, d_symbols, 0, frames, 0, n_steps, L, d_workspace, workspace_bytes, nullptr, d_final_metrics,
                             d_renorm_sum, d_start_state, stream);
}

int vit_hip_update_batch_resume(vit_hip_handle h, const void* d_symbols, size_t symbol_frame_stride, size_t frames,
                                size_t first_step, size_t n_steps, size_t L, void* d_workspace, size_t workspace_bytes,
                                void* d_metrics_inout, uint64_t* d_renorm_sum, vit_hip_stream_t stream) {
    if (!d_metrics_inout) return fail(VIT_HIP_ERR_INVALID_ARG, "d_metrics_inout is NULL (vit_hip_reset_batch fills it for step 0)");
    return update_batch_impl(h, d_symbols, symbol_frame_stride, frames, first_step, n_steps, L, d_workspace, workspace_bytes,
                             d_metrics_inout, d_metrics_inout, d_renorm_sum, nullptr, stream);
}

int vit_hip_chainback_batch(vit_hip_handle h, const void* d_workspace, size_t frames, size_t L, uint8_t* d_bytes_out,
                            const uint32_t* d_end_state, vit_hip_stream_t stream) {
    return chainback_batch_impl(h, d_workspace, frames, L, d_bytes_out, d_end_state, stream, 0);
}

int vit_hip_chainback_batch_ex(vit_hip_handle h, const void* d_workspace, size_t frames, size_t L, uint8_t* d_bytes_out,
                               const uint32_t* d_end_state, vit_hip_stream_t stream, int kernel) {
    if (kernel != VIT_HIP_KERNEL_CHAINBACK && kernel != VIT_HIP_KERNEL_CHAINBACK_ALT)
        return fail(VIT_HIP_ERR_INVALID_ARG, "kernel must be VIT_HIP_KERNEL_CHAINBACK or VIT_HIP_KERNEL_CHAINBACK_ALT");
    return chainback_batch_impl(h, d_workspace, frames, L, d_bytes_out, d_end_state, stream, 0, kernel == VIT_HIP_KERNEL_CHAINBACK_ALT);
}

int vit_hip_decode_batch(vit_hip_handle h, const void* d_symbols, size_t frames, size_t L, void* d_workspace,
                         size_t workspace_bytes, uint8_t* d_bytes_out, void* d_final_metrics, uint64_t* d_renorm_sum,
                         const uint32_t* d_end_state, vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    const int rc = vit_hip_update_batch(h, d_symbols, frames, L + (size_t)h->K - 1, L, d_workspace, workspace_bytes,
                                        d_final_metrics, d_renorm_sum, nullptr, stream);
    if (rc != VIT_HIP_OK) return rc;
    return vit_hip_chainback_batch(h, d_workspace, frames, L, d_bytes_out, d_end_state, stream);
}

int vit_hip_export_decisions(vit_hip_handle h, const void* d_workspace, size_t frames, size_t n_steps, size_t L,
                             uint64_t* d_decisions, vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (frames == 0 || n_steps == 0) return VIT_HIP_OK;
    if (!d_workspace || !d_decisions) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL buffer");
    if (n_steps > L + (size_t)h->K - 1) return fail(VIT_HIP_ERR_INVALID_ARG, "n_steps exceeds traceback length + K-1");
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    switch (h->plan) {
        case VIT_HIP_PLAN_REG: return launched(h, reg_export(h->reg_code, d_workspace, frames, n_steps, L, d_decisions, st), "export");
        case VIT_HIP_PLAN_LDS2: return launched(h, lds2_export(h->K, d_workspace, frames, n_steps, L, d_decisions, st), "export");
        default: {
            const size_t rows = L + (size_t)h->K - 1;
            const size_t W8 = (size_t)h->W * 8;
            VIT_HIP_CHECK(hipMemcpy2DAsync(d_decisions, n_steps * W8, d_workspace, rows * W8, n_steps * W8, frames,
                                           hipMemcpyDeviceToDevice, st));
            return VIT_HIP_OK;
        }
    }
}

int vit_hip_depuncture_batch(vit_hip_handle h, const void* d_punctured, size_t punctured_per_frame,
                             const int32_t* d_source_index, size_t symbols_per_frame, size_t frames, void* d_symbols_out,
                             vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (frames == 0 || symbols_per_frame == 0) return VIT_HIP_OK;
    if (!d_punctured || !d_source_index || !d_symbols_out) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL buffer");
    if (symbols_per_frame % (size_t)h->R != 0)
        return fail(VIT_HIP_ERR_INVALID_ARG, "symbols_per_frame must be a multiple of the code rate R");
    const size_t chunks = (symbols_per_frame + 7) / 8;
    if (frames > 0x7FFFFFFFull * 256ull / chunks) return fail(VIT_HIP_ERR_INVALID_ARG, "batch too large for one launch");
    const size_t sb = (size_t)h->soft_bytes;
    if (misaligned(d_punctured, sb) || misaligned(d_symbols_out, sb))
        return fail(VIT_HIP_ERR_INVALID_ARG, "d_punctured and d_symbols_out must be aligned to the symbol type");
    if (misaligned(d_source_index, sizeof(int32_t))) return fail(VIT_HIP_ERR_INVALID_ARG, "d_source_index must be aligned to 4 bytes");
    // the extents the kernel can touch (the map is bounded by punctured_per_frame on the device); an input too large to state is "all of memory"
    const size_t out_b = frames * symbols_per_frame * sb;
    const size_t in_b = punctured_per_frame > (size_t)-1 / sb / frames ? (size_t)-1 - (uintptr_t)d_punctured : frames * punctured_per_frame * sb;
    if (overlap(d_symbols_out, out_b, d_punctured, in_b)) return fail(VIT_HIP_ERR_INVALID_ARG, "d_symbols_out overlaps d_punctured");
    if (overlap(d_symbols_out, out_b, d_source_index, symbols_per_frame * sizeof(int32_t)))
        return fail(VIT_HIP_ERR_INVALID_ARG, "d_symbols_out overlaps d_source_index");
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((chunks * frames + 255) / 256);
    if (h->soft_bytes == 2)
        hipLaunchKernelGGL(vit::depuncture_kernel<int16_t>, dim3(blocks), dim3(256), 0, st, (const int16_t*)d_punctured,
                           punctured_per_frame, d_source_index, symbols_per_frame, frames, (int16_t*)d_symbols_out);
    else
        hipLaunchKernelGGL(vit::depuncture_kernel<int8_t>, dim3(blocks), dim3(256), 0, st, (const int8_t*)d_punctured,
                           punctured_per_frame, d_source_index, symbols_per_frame, frames, (int8_t*)d_symbols_out);
    VIT_HIP_CHECK(hipGetLastError());
    return VIT_HIP_OK;
}

int vit_hip_reset_batch(vit_hip_handle h, size_t frames, const uint32_t* d_start_state, void* d_metrics,
                        vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (frames == 0) return VIT_HIP_OK;
    if (!d_metrics) return fail(VIT_HIP_ERR_INVALID_ARG, "d_metrics is NULL");
    const size_t total = frames * (size_t)h->N;
    if (total > 0x7FFFFFFFull * 256ull) return fail(VIT_HIP_ERR_INVALID_ARG, "batch too large for one launch");
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (h->error_bytes == 2)
        hipLaunchKernelGGL(vit::reset_kernel<uint16_t>, dim3(blocks), dim3(256), 0, st, (uint16_t*)d_metrics, d_start_state,
                           frames, (uint32_t)h->N, h->cfg_raw[1], h->cfg_raw[2]);
    else
        hipLaunchKernelGGL(vit::reset_kernel<uint8_t>, dim3(blocks), dim3(256), 0, st, (uint8_t*)d_metrics, d_start_state,
                           frames, (uint32_t)h->N, h->cfg_raw[1], h->cfg_raw[2]);
    VIT_HIP_CHECK(hipGetLastError());
    return VIT_HIP_OK;
}

static int vit_hip_get_kernel_resources_impl(vit_hip_handle h, int kernel, vit_hip_kernel_resources* out) {
    if (!h || !out) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL argument");
    memset(out, 0, sizeof(*out));
    kd::KernelResources r;
    unsigned dyn = 0;
    bool found = false;
    switch (h->plan) {
        case VIT_HIP_PLAN_REG:
            if (kernel < VIT_HIP_KERNEL_UPDATE || kernel > VIT_HIP_KERNEL_RESUME) return fail(VIT_HIP_ERR_INVALID_ARG, "unknown kernel");
            found = reg_kernel_resources(h->reg_code, h->shift, kernel, &r, &dyn);
            break;
        case VIT_HIP_PLAN_LDS2:
            if (kernel != VIT_HIP_KERNEL_UPDATE && kernel != VIT_HIP_KERNEL_CHAINBACK) return fail(VIT_HIP_ERR_INVALID_ARG, "unknown kernel");
            found = lds2_kernel_resources(h->K, h->R, h->shift, kernel == VIT_HIP_KERNEL_UPDATE, &r, &dyn);
            break;
        default: return fail(VIT_HIP_ERR_UNSUPPORTED, "kernel resources are reported for the register plan and PLAN_LDS2");
    }
    if (!found) return fail(VIT_HIP_ERR_RUNTIME, "kernel descriptor not found in the library's code objects");
    kernel_resources_to_abi(r, dyn, out);
    return VIT_HIP_OK;
}

int vit_hip_get_kernel_resources(vit_hip_handle h, int kernel, vit_hip_kernel_resources* out) {
    VIT_HIP_NOTHROW(return vit_hip_get_kernel_resources_impl(h, kernel, out));
}

#ifdef VIT_HIP_CLOCK_STAMPS
// measurement build only (include/vit_hip_experiments.h): every register-plan update launched from now on stamps into d_stamps
// ([tiles][6] uint64: shader clock and constant clock at entry, at exit, XCC id, HW id); NULL switches it off
int vit_hip_experiment_clock_stamps(void* d_stamps) {
    vit::g_clock_stamps = (uint64_t*)d_stamps;
    return VIT_HIP_OK;
}
#endif

}  // extern "C"
