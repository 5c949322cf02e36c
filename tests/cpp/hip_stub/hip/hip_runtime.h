// <hip/hip_runtime.h> for a HOST build of a kernel header (tests/cpp/crc_host_check.cpp): the built-ins a kernel's source names, stubbed
// so that g++ compiles it and a program runs it ONE thread per block.  Nothing of the HIP runtime is behind these names.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __launch_bounds__(...)

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
static dim3 threadIdx(0), blockIdx(0), blockDim(1), gridDim(1);      // one thread per block: the program sets blockIdx / gridDim
inline void __syncthreads() {}
inline uint32_t __shfl_xor(uint32_t v, int) { return v; }            // a wave of one lane: the program does the exchange itself

typedef void* hipStream_t;
enum hipError_t { hipSuccess = 0 };
inline hipError_t hipGetLastError() { return hipSuccess; }
#define hipLaunchKernelGGL(...) ((void)0)
