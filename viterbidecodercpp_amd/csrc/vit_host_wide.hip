// vit_host_wide.hip -- the single-frame kernels of K = 8, 9 with R <= 4 (kernels_one.hpp: one_update_wide_kernel,
// one_frame_wide_kernel, one_chainback_wide_kernel) and their launchers, which vit_host.hip calls.  A unit of its own for the build's
// sake only: vit_host.hip is the longest compile of the library, and these kernels compile beside it instead of behind it.
#define VIT_ONE_WIDE_UNIT       // kernels_one.hpp: the K <= 7 chainback kernel (no template) belongs to vit_host.hip
#include "vit_internal.hpp"
#include "kernels_one.hpp"

namespace vit {

namespace {
// (K, R, width) known at run time as template arguments: f(kernel-of<K, R, SHIFT>) for K = 8, 9 and R = 1..4
template <class F>
hipError_t with_wide_code(int K, int R, int shift, F&& f) {
    if ((K != 8 && K != 9) || R < 1 || R > 4) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    (void)with_rate(R, -1, [&](auto r) {
        if constexpr (r() <= 4) {
            if (K == 8) e = shift ? f(std::integral_constant<int, 8>{}, r, std::integral_constant<int, 8>{}) : f(std::integral_constant<int, 8>{}, r, std::integral_constant<int, 0>{});
            else e = shift ? f(std::integral_constant<int, 9>{}, r, std::integral_constant<int, 8>{}) : f(std::integral_constant<int, 9>{}, r, std::integral_constant<int, 0>{});
        }
        return 0;
    });
    return e;
}
}  // namespace

hipError_t one_wide_launch_update(int K, int R, int shift, const OneUpdateWideArgs& a, hipStream_t st) {
    return with_wide_code(K, R, shift, [&](auto k, auto r, auto s) {
        hipLaunchKernelGGL((one_update_wide_kernel<k(), r(), s()>), dim3(1), dim3(64), 0, st, a);
        return hipGetLastError();
    });
}

hipError_t one_wide_launch_frame(int K, int R, int shift, const OneFrameWideArgs& a, hipStream_t st) {
    const size_t smem = a.do_chainback ? one_chainback_wide_lds_bytes(K == 8 ? 2 : 4) : 0;
    return with_wide_code(K, R, shift, [&](auto k, auto r, auto s) {
        auto kern = one_frame_wide_kernel<k(), r(), s()>;
        if (smem > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(1), dim3(64), smem, st, a);
        return hipGetLastError();
    });
}

hipError_t one_wide_launch_chainback(int words_per_row, const OneChainbackArgs& a, hipStream_t st) {
    auto launch = [&](auto kern, size_t smem) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(1), dim3(64), smem, st, a);
        return hipGetLastError();
    };
    if (words_per_row == 2) return launch(one_chainback_wide_kernel<2>, one_chainback_wide_lds_bytes(2));
    if (words_per_row == 4) return launch(one_chainback_wide_kernel<4>, one_chainback_wide_lds_bytes(4));
    return hipErrorInvalidValue;
}

}  // namespace vit
