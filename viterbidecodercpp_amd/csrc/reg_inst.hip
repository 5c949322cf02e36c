// reg_inst.hip -- one stock PLAN_REG code per translation unit: compile with -DVIT_REG_ID=<an id of VIT_REG_STOCK_CODES> (see Makefile).
#include "reg_plan.hpp"

namespace vit {
using SP = RegSpecOf<VIT_REG_ID>::type;

template <> int reg_launch_update<VIT_REG_ID>(int shift, const RegUpdateArgs& a, unsigned tiles, hipStream_t st) {
    if (a.metrics_in) {
        if (shift) hipLaunchKernelGGL((reg_resume_kernel<SP, 8>), dim3(tiles), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((reg_resume_kernel<SP, 0>), dim3(tiles), dim3(64), 0, st, a);
    } else {
        if (shift) hipLaunchKernelGGL((reg_update_kernel<SP, 8>), dim3(tiles), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((reg_update_kernel<SP, 0>), dim3(tiles), dim3(64), 0, st, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <> int reg_launch_chainback<VIT_REG_ID>(const RegChainbackArgs& a, unsigned tiles, hipStream_t st, bool coop) {
    constexpr unsigned FPB = reg_chainback_frames_per_block(SP::K);
    if (coop && SP::NREG == 64) hipLaunchKernelGGL(reg_chainback_alt_kernel<SP>, dim3(tiles), dim3(64), 0, st, a);
    else if (coop && SP::NREG == 16 && SP::LANE_BITS == 2) hipLaunchKernelGGL(reg_chainback_alt_kernel<SP>, dim3((a.frames + 127) / 128), dim3(64), reg_chainback_dyn_lds_bytes(SP::K, SP::R, true), st, a);
    else hipLaunchKernelGGL(reg_chainback_kernel<SP>, dim3((a.frames + FPB - 1) / FPB), dim3(64), reg_chainback_dyn_lds_bytes(SP::K, SP::R, false), st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <> int reg_launch_export<VIT_REG_ID>(const RegExportArgs& a, unsigned blocks, hipStream_t st) {
    hipLaunchKernelGGL(reg_export_kernel<SP>, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace vit
