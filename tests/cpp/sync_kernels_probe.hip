// sync_kernels_probe.hip -- test infrastructure for tests/test_gpu_sync_kernels.py: the two small kernels of node synchronisation
// (sync_state_kernel, sync_pick_kernel of csrc/kernels_sync.hpp) on inputs a real search never produces.  The kernels and their
// launchers are the library's own, compiled from its header; this file only walks over the sets.  Every set has SYNC_MAX_HYPOTHESES
// slots in each of its arrays, whatever its n_hyp; a set with n_hyp == 0 is not launched.  The per-set parameters are host arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../viterbidecodercpp_amd/csrc/kernels_sync.hpp"

extern "C" {

// set s: d_errors / d_compared + s * 64 -> d_best[s].  0, or -1 when a launch failed
int sync_probe_pick(const uint32_t* d_errors, const uint32_t* d_compared, uint32_t* d_best, const uint32_t* n_hyp, uint32_t n_sets,
                    void* stream) {
    for (uint32_t s = 0; s < n_sets; ++s) {
        if (n_hyp[s] == 0) continue;
        if (n_hyp[s] > vit::SYNC_MAX_HYPOTHESES) return -1;
        vit::SyncPickArgs a{};
        a.errors = d_errors + (size_t)s * vit::SYNC_MAX_HYPOTHESES;
        a.compared = d_compared + (size_t)s * vit::SYNC_MAX_HYPOTHESES;
        a.best = d_best + s;
        a.n_hyp = n_hyp[s];
        if (vit::sync_launch_pick(a, (hipStream_t)stream) != 0) return -1;
    }
    return 0;
}

// set s: the decoded bytes of hypothesis h at d_bytes + s * set_bytes + h * byte_stride[s] -> d_state / d_errors / d_compared + s * 64
int sync_probe_state(const uint8_t* d_bytes, uint64_t set_bytes, uint32_t* d_state, uint32_t* d_errors, uint32_t* d_compared,
                     const uint64_t* byte_stride, const uint32_t* n_hyp, const uint32_t* skip_bytes, const uint32_t* K, uint32_t n_sets,
                     void* stream) {
    for (uint32_t s = 0; s < n_sets; ++s) {
        if (n_hyp[s] == 0) continue;
        // what the kernel reads stays inside the set's bytes
        if (n_hyp[s] > vit::SYNC_MAX_HYPOTHESES || skip_bytes[s] == 0 || (n_hyp[s] - 1) * byte_stride[s] + skip_bytes[s] > set_bytes) return -1;
        vit::SyncStateArgs a{};
        a.bytes = d_bytes + (size_t)s * set_bytes;
        a.state = d_state + (size_t)s * vit::SYNC_MAX_HYPOTHESES;
        a.errors = d_errors + (size_t)s * vit::SYNC_MAX_HYPOTHESES;
        a.compared = d_compared + (size_t)s * vit::SYNC_MAX_HYPOTHESES;
        a.byte_stride = byte_stride[s];
        a.n_hyp = n_hyp[s]; a.skip_bytes = skip_bytes[s]; a.K = K[s];
        if (vit::sync_launch_state(a, (hipStream_t)stream) != 0) return -1;
    }
    return 0;
}

}  // extern "C"
