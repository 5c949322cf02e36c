// common.hpp -- types shared by the kernel plans.
#pragma once
#include <stdint.h>

namespace vit {

// Decoder constants in the device's 16-bit domain: every value is (reference value << shift), shift = 0 for
// (int16_t,uint16_t) and 8 for (int8_t,uint8_t).
struct DevConfig {
    uint16_t max_error, init_start, init_non_start, threshold;
    int16_t high, low;
};

// the branch error of one symbol, shared by the LDS plan and the single-frame kernels
__device__ __forceinline__ uint16_t abs_soft(int32_t expected, int32_t y) {
    // const soft_t error = expected - sym; error_t(get_abs(error))   (viterbi_decoder_scalar.h:68-71, :155-159)
    const int16_t d = (int16_t)(expected - y);
    const int16_t n = (int16_t)(-(int32_t)d);
    return (uint16_t)(d > 0 ? d : n);
}

}  // namespace vit
