// kernels_depuncture.hpp -- the depuncturing gather of vit_hip_depuncture_batch (include/vit_hip.h), included only from vit_hip.hip.
// It stands in a header of its own so that a host program can compile it with the HIP built-ins stubbed
// (tests/cpp/depuncture_host_check.cpp), as the kernels of the later routes are.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace vit {
// depuncturing gather (examples/helpers/puncture_code_helpers.h:17-55 for a batch): out[f][k] = in[f][idx[k]] or 0.  One
// thread makes 8 consecutive output symbols of one frame (16-byte / 8-byte store); the index map is read once per 8 symbols
// as two 16-byte loads and stays in L2; source reads are consecutive where the map is monotonic.
// in_stride is punctured_per_frame: the frame's stride AND the bound of the map.  An entry j selects src[j] only where 0 <= j and
// (size_t)j < in_stride; every other entry reads as the erasure 0, so that whatever the map memory holds, nothing outside
// in[0 .. frames * in_stride) is read (the host cannot check a map that lives in device memory).
template <typename T>
__global__ void depuncture_kernel(const T* __restrict__ in, size_t in_stride, const int32_t* __restrict__ idx, size_t n_out,
                                  size_t frames, T* __restrict__ out) {
    const size_t chunks = (n_out + 7) / 8;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= chunks * frames) return;
    const size_t f = gid / chunks, k0 = (gid % chunks) * 8;
    const T* src = in + f * in_stride;
    T* dst = out + f * n_out + k0;
    T v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const size_t k = k0 + i;
        const int32_t j = k < n_out ? idx[k] : -1;
        v[i] = (j >= 0 && (size_t)j < in_stride) ? src[j] : (T)0;
    }
    if (k0 + 8 <= n_out && ((uintptr_t)dst % (8 * sizeof(T))) == 0) {
        typedef T vec8 __attribute__((vector_size(8 * sizeof(T))));      // the spelling g++ takes too: the same <8 x T> to hipcc
        vec8 w;
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = v[i];
        *(vec8*)dst = w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (k0 + i < n_out) dst[i] = v[i];
    }
}
}  // namespace vit
