// vit_tools.hip -- what surrounds decoding: synthetic frames and bit-error counts on the device (kernels_synth.hpp), the shader
// clock probe, the listing of the library's kernels, install-time compilation of register-plan kernels, and the RCCL broadcast of
// the shared table.
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <mutex>

#include "vit_internal.hpp"
#include "kernels_synth.hpp"
#include "reg_jit.hpp"

using namespace vit;

extern "C" {

int vit_hip_synth_batch(vit_hip_handle h, size_t frames, size_t L, uint64_t seed, uint64_t first_frame, float ebn0_db,
                        int noise_free, uint8_t* d_tx_bytes, void* d_symbols, vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (frames == 0) return VIT_HIP_OK;
    if (!d_symbols) return fail(VIT_HIP_ERR_INVALID_ARG, "d_symbols is NULL");
    if (L % 8 != 0) return fail(VIT_HIP_ERR_INVALID_ARG, "L must be a multiple of 8 (whole info bytes)");
    if (!h->linear) return fail(VIT_HIP_ERR_UNSUPPORTED, "the branch table is not that of a convolutional code (no polynomials)");
    if (h->soft_bytes == 2 && misaligned(d_symbols, 2)) return fail(VIT_HIP_ERR_INVALID_ARG, "int16 symbols must be 2-byte aligned");
    const size_t S = L + (size_t)h->K - 1;
    const size_t chunks = (S + 7) / 8;
    if (frames > 0xFFFFFFFFull || S > 0x0FFFFFFFull || chunks * frames > 0x7FFFFFFFull * 256ull)
        return fail(VIT_HIP_ERR_INVALID_ARG, "batch too large for one launch");
    SynthArgs a{};
    a.tx = d_tx_bytes;
    a.symbols = d_symbols;
    a.seed = seed;
    a.first_frame = first_frame;
    a.frames = (uint32_t)frames; a.L = (uint32_t)L; a.S = (uint32_t)S; a.K = (uint32_t)h->K; a.R = (uint32_t)h->R;
    for (int i = 0; i < h->R && i < 8; ++i) a.G[i] = h->G[i];
    a.high = h->high; a.low = h->low;
    a.noise_free = noise_free ? 1 : 0;
    // run_snr_ber.cpp:311-330, in float like the reference
    const float EsNo_dB = ebn0_db - 10.0f * log10f((float)h->R);
    const float noise_variance = powf(10.0f, -(EsNo_dB + 3.0f) / 10.0f);
    a.sigma = sqrtf(noise_variance);
    a.mean = ((float)h->high + (float)h->low) / 2.0f;
    a.scale = (((float)h->high - (float)h->low) / 2.0f) * (1.0f / sqrtf(1.0f + noise_variance));
    VIT_HIP_ON_DEVICE(h->device);
    const unsigned blocks = (unsigned)((chunks * frames + 255) / 256);
    const int rc = with_rate(h->R, -1, [&](auto r) {
        if (h->soft_bytes == 2) hipLaunchKernelGGL((synth_kernel<int16_t, r()>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((synth_kernel<int8_t, r()>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
    if (rc != 0) return fail(VIT_HIP_ERR_RUNTIME, "synth kernel launch failed");
    return VIT_HIP_OK;
}

int vit_hip_count_bit_errors(vit_hip_handle h, const uint8_t* d_a, const uint8_t* d_b, size_t n_bytes, uint64_t* d_count,
                             vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (n_bytes == 0) return VIT_HIP_OK;
    if (!d_a || !d_b || !d_count) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL buffer");
    VIT_HIP_ON_DEVICE(h->device);
    BitErrArgs a{d_a, d_b, n_bytes, (unsigned long long*)d_count};
    size_t blocks = (n_bytes / 16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bit_errors_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    VIT_HIP_CHECK(hipGetLastError());
    return VIT_HIP_OK;
}

static int vit_hip_shader_clock_mhz_impl(int device, double* mhz_out, double* cycles_per_pk_instr_out) {
    if (!mhz_out) return fail(VIT_HIP_ERR_INVALID_ARG, "mhz_out is NULL");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VIT_HIP_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(VIT_HIP_ERR_INVALID_ARG, "device index out of range");
    VIT_HIP_ON_DEVICE(device);
    int cus = 0, wall_khz = 0;
    VIT_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || wall_khz <= 0) wall_khz = 100000;
    // with the issue rate asked for: four waves on every SIMD of the chip (one 256-thread workgroup per SIMD), about 2 ms of
    // packed adds at 2.4 GHz.  Clock only: ONE wave per CU -- a probe that can run beside other kernels without adding a chip
    // full of vector work to their power draw (the card lowers its clock under it: 1.96 GHz read by the heavy probe beside the
    // K7 pipeline against 2.3 GHz by this one)
    const bool light = cycles_per_pk_instr_out == nullptr;
    const unsigned threads = light ? 64u : 256u;
    const unsigned blocks = (unsigned)(cus > 0 ? cus : 256) * (light ? 1u : 4u), iters = 4000;
    const size_t waves = (size_t)blocks * (threads / 64u);
    uint64_t* d_out = nullptr;
    VIT_HIP_CHECK(hipMalloc((void**)&d_out, waves * 2 * sizeof(uint64_t)));
    std::vector<uint64_t> host(waves * 2);
    hipLaunchKernelGGL(shader_clock_kernel, dim3(blocks), dim3(threads), 0, nullptr, d_out, iters, 3u);
    const hipError_t e1 = hipGetLastError();
    const hipError_t e2 = hipMemcpy(host.data(), d_out, waves * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(VIT_HIP_ERR_RUNTIME, "shader clock kernel failed");
    std::vector<double> ratio, cyc;
    for (size_t w = 0; w < waves; ++w)
        if (host[2 * w + 1] > 0) {
            ratio.push_back((double)host[2 * w] / (double)host[2 * w + 1]);
            cyc.push_back((double)host[2 * w] / ((double)iters * 64.0));
        }
    if (ratio.empty()) return fail(VIT_HIP_ERR_RUNTIME, "shader clock kernel returned no samples");
    std::sort(ratio.begin(), ratio.end());
    std::sort(cyc.begin(), cyc.end());
    *mhz_out = ratio[ratio.size() / 2] * (double)wall_khz / 1000.0;
    // four waves share a SIMD: the SIMD issues one of these instructions every (wave cycles per instruction) / 4
    if (cycles_per_pk_instr_out) *cycles_per_pk_instr_out = cyc[cyc.size() / 2] / 4.0;
    return VIT_HIP_OK;
}

int vit_hip_shader_clock_mhz(int device, double* mhz_out, double* cycles_per_pk_instr_out) {
    VIT_HIP_NOTHROW(return vit_hip_shader_clock_mhz_impl(device, mhz_out, cycles_per_pk_instr_out));
}

static int vit_hip_list_kernels_impl(size_t index, char* name, size_t name_capacity, vit_hip_kernel_resources* out) {
    const kd::Table& t = kd::own_library();
    if (t.empty()) return fail(VIT_HIP_ERR_RUNTIME, "the library's own file could not be read for its kernel descriptors");
    if (index >= t.size()) return fail(VIT_HIP_ERR_INVALID_ARG, "index past the last kernel");
    if (name && name_capacity > 0) {
        const size_t n = t[index].first.size() < name_capacity - 1 ? t[index].first.size() : name_capacity - 1;
        memcpy(name, t[index].first.data(), n);
        name[n] = 0;
    }
    if (out) kernel_resources_to_abi(t[index].second, 0, out);
    return VIT_HIP_OK;
}

int vit_hip_list_kernels(size_t index, char* name, size_t name_capacity, vit_hip_kernel_resources* out) {
    VIT_HIP_NOTHROW(return vit_hip_list_kernels_impl(index, name, name_capacity, out));
}

static int vit_hip_precompile_impl(int K, int R, const uint32_t* polynomials, int soft_bytes, const char* directory, char* path_out,
                                   size_t path_capacity) {
    if (!polynomials) return fail(VIT_HIP_ERR_INVALID_ARG, "polynomials is NULL");
    if (soft_bytes != 1 && soft_bytes != 2) return fail(VIT_HIP_ERR_UNSUPPORTED, "soft_bytes must be 1 or 2");
    if (!reg_jit_supported(K, R)) return fail(VIT_HIP_ERR_UNSUPPORTED, "the register plan serves K = 2..9 with R <= 6");
    // the same normal form vit_hip_create recovers from a branch table: bit 0 and bit K-1 of every polynomial set
    uint32_t G[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < R; ++i) G[i] = (polynomials[i] & ((1u << K) - 1u)) | 1u | (1u << (K - 1));
    // all polynomials zero: the GENERIC kernels of (K, R), which read the polynomials from their arguments (RegSpec::GENERIC)
    bool generic = true;
    for (int i = 0; i < R; ++i) generic = generic && polynomials[i] == 0;
    if (generic) {
        if (!reg_generic_supported(K, R)) return fail(VIT_HIP_ERR_UNSUPPORTED, "generic register-plan kernels exist for K = 3..9 with R = 1..4 (not K = 6 at an odd R)");
        for (int i = 0; i < R; ++i) G[i] = 0;
    }
    std::string err;
    const int shift = soft_bytes == 1 ? 8 : 0;
    const std::string name = reg_jit_object_name(K, R, G, shift, err);
    if (name.empty()) return fail(VIT_HIP_ERR_RUNTIME, err);
    const std::string dir = directory && *directory ? std::string(directory) : package_cache_dir();
    (void)mkdir(dir.c_str(), 0755);
    const std::string path = dir + "/" + name;
    struct stat st;
    if (!(stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) && !reg_jit_compile(K, R, G, shift, path, err))
        return fail(VIT_HIP_ERR_RUNTIME, err);
    if (path_out && path_capacity) snprintf(path_out, path_capacity, "%s", path.c_str());
    return VIT_HIP_OK;
}

int vit_hip_precompile(int K, int R, const uint32_t* polynomials, int soft_bytes, const char* directory, char* path_out, size_t path_capacity) {
    VIT_HIP_NOTHROW(return vit_hip_precompile_impl(K, R, polynomials, soft_bytes, directory, path_out, path_capacity));
}

// ---- RCCL broadcast of the shared table (the one collective of the multi-GPU path) ----
namespace {
typedef int (*nccl_broadcast_fn)(const void*, void*, size_t, int /*ncclDataType_t*/, int, void* /*ncclComm_t*/, hipStream_t);
typedef const char* (*nccl_errstr_fn)(int);
struct RcclApi {
    nccl_broadcast_fn broadcast = nullptr;
    nccl_errstr_fn errstr = nullptr;
};
// The communicator belongs to the RCCL the host program uses: take the symbol from the process first (a C/C++ host that
// links -lrccl), and load librccl.so only when the process does not export it.
const RcclApi* rccl_api() {
    // resolved exactly once, by whichever thread gets here first (function-local static: the others wait for the
    // initialiser to finish and then see the filled table -- one host thread per GPU calls this at the same moment)
    static const RcclApi api = [] {
        RcclApi a;
        void* sym = dlsym(RTLD_DEFAULT, "ncclBroadcast");
        void* lib = nullptr;
        if (!sym) {
            const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
            for (const char* n : names) {
                lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
                if (lib) break;
            }
            if (lib) sym = dlsym(lib, "ncclBroadcast");
        }
        a.broadcast = (nccl_broadcast_fn)sym;
        a.errstr = (nccl_errstr_fn)(lib ? dlsym(lib, "ncclGetErrorString") : dlsym(RTLD_DEFAULT, "ncclGetErrorString"));
        return a;
    }();
    return api.broadcast ? &api : nullptr;
}

constexpr size_t BROADCAST_STAGING_BYTES = 264 * 1024;      // >= vit_hip_blob_bytes(16, 8, 2, 2)
struct BroadcastStaging { void* buf[64] = {nullptr}; std::mutex alloc; std::mutex use[64]; };
BroadcastStaging* broadcast_staging_table() { static BroadcastStaging t; return &t; }
// the calling thread has `device` current (DeviceGuard); nullptr if the device index is out of the table or the one-off hipMalloc fails
void* broadcast_staging(int device) {
    if (device < 0 || device >= 64) return nullptr;
    BroadcastStaging& t = *broadcast_staging_table();
    std::lock_guard<std::mutex> lock(t.alloc);
    if (!t.buf[device] && hipMalloc(&t.buf[device], BROADCAST_STAGING_BYTES) != hipSuccess) { t.buf[device] = nullptr; (void)hipGetLastError(); }
    return t.buf[device];
}
std::mutex* broadcast_staging_mutex(int device) { return &broadcast_staging_table()->use[device]; }
}  // namespace

static int vit_hip_broadcast_table_impl(void* nccl_comm, int root, int rank, int K, int R, int soft_bytes, int error_bytes,
                            void* branch_table, void* config, int device, vit_hip_stream_t stream) {
    // Argument checks depend only on what every rank passes alike (K, R, widths, pointers being non-NULL): a bad call fails on
    // all ranks the same way and nobody is left waiting in ncclBroadcast.  Past them, a rank enters the collective exactly once
    // whatever happens to its DATA: a root that cannot pack or upload its table broadcasts a poisoned header, which the other
    // ranks report as an error.  What a rank cannot do is take part without a device: hipSetDevice failing on ONE rank (or, at
    // the process's FIRST broadcast on that device only, the one-off hipMalloc of the 264 KiB staging buffer) returns
    // VIT_HIP_ERR_NO_DEVICE from that rank BEFORE the collective, and the other ranks wait in ncclBroadcast until the caller aborts
    // the communicator (ncclCommAbort) -- the usual contract of a rank that dies in front of a collective; include/vit_hip.h says so.
    if (!nccl_comm || !branch_table || !config) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL argument");
    if (K < 2 || K > 16 || R < 1 || R > 8 || !((soft_bytes == 2 && error_bytes == 2) || (soft_bytes == 1 && error_bytes == 1)))
        return fail(VIT_HIP_ERR_UNSUPPORTED, "unsupported (K, R, soft_t, error_t)");
    const size_t need = vit_hip_blob_bytes(K, R, soft_bytes, error_bytes);
    if (need > BROADCAST_STAGING_BYTES) return fail(VIT_HIP_ERR_UNSUPPORTED, "blob larger than the staging buffer");
    const RcclApi* api = rccl_api();
    if (!api) return fail(VIT_HIP_ERR_RUNTIME, "RCCL not available: ncclBroadcast is neither in the process nor in librccl.so");
    std::vector<uint8_t> blob(need, 0);
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(VIT_HIP_ERR_NO_DEVICE, "hipSetDevice failed on this rank BEFORE the broadcast: abort the communicator, the other ranks are waiting in it");
    hipStream_t st = (hipStream_t)stream;
    // the staging buffer: allocated ONCE per device, at the first call, for the largest blob the library accepts (K = 16, R = 8,
    // 16-bit: 256 KiB + header) and kept for the life of the process -- a later broadcast cannot fail in front of the collective
    // for want of memory; the only pre-collective failure left is a rank without a usable device
    void* d_buf = broadcast_staging(device);
    if (!d_buf)
        return fail(VIT_HIP_ERR_NO_DEVICE, "no staging buffer on this rank's device BEFORE the broadcast (first call: hipMalloc of 264 KiB failed): abort the communicator, the other ranks are waiting in it");
    // one broadcast at a time per device buffer
    std::lock_guard<std::mutex> staging_lock(*broadcast_staging_mutex(device));
    std::string root_error;
    if (rank == root) {
        if (vit_hip_pack_blob(K, R, soft_bytes, error_bytes, branch_table, config, blob.data(), need) != VIT_HIP_OK) {
            root_error = last_error();
            memset(blob.data(), 0, sizeof(BlobHeader));          // poisoned: magic 0
        }
        if (hipMemcpyAsync(d_buf, blob.data(), need, hipMemcpyHostToDevice, st) != hipSuccess) {
            root_error = "hipMemcpyAsync (blob to device) failed";
            (void)hipGetLastError();
            (void)hipMemset(d_buf, 0, sizeof(BlobHeader));       // poison through the null stream, not the one that just failed
        }
    }
    int result = VIT_HIP_OK;
    const int nrc = api->broadcast(d_buf, d_buf, need, 1 /* ncclUint8 */, root, nccl_comm, st);
    if (nrc != 0)
        result = fail(VIT_HIP_ERR_RUNTIME, std::string("ncclBroadcast: ") + (api->errstr ? api->errstr(nrc) : "error"));
    else if (hipMemcpyAsync(blob.data(), d_buf, need, hipMemcpyDeviceToHost, st) != hipSuccess ||
             hipStreamSynchronize(st) != hipSuccess)
        result = fail(VIT_HIP_ERR_RUNTIME, "copying the broadcast blob back failed");
    if (result != VIT_HIP_OK) return result;
    if (!root_error.empty()) return fail(VIT_HIP_ERR_RUNTIME, "root rank could not pack the table: " + root_error);
    BlobHeader hd;
    memcpy(&hd, blob.data(), sizeof(hd));
    if (hd.magic != BLOB_MAGIC) return fail(VIT_HIP_ERR_RUNTIME, "the root rank failed to pack its table (poisoned header received)");
    if (hd.K != K || hd.R != R || hd.soft_bytes != soft_bytes || hd.error_bytes != error_bytes)
        return fail(VIT_HIP_ERR_INVALID_ARG, "the root rank broadcast a table for a different (K, R, soft_t, error_t)");
    if (rank != root) {
        const size_t tb = need - sizeof(hd) - 4 * (size_t)error_bytes;
        memcpy(branch_table, blob.data() + sizeof(hd), tb);
        memcpy(config, blob.data() + sizeof(hd) + tb, 4 * (size_t)error_bytes);
    }
    return VIT_HIP_OK;
}


int vit_hip_broadcast_table(void* nccl_comm, int root, int rank, int K, int R, int soft_bytes, int error_bytes,
                            void* branch_table, void* config, int device, vit_hip_stream_t stream) {
    VIT_HIP_NOTHROW(return vit_hip_broadcast_table_impl(nccl_comm, root, rank, K, R, soft_bytes, error_bytes, branch_table, config, device, stream));
}

}  // extern "C"
