// reg_plan.hpp -- host side of PLAN_REG: the list of stock codes, launchers, workspace geometry, residency rules.
//
// The device code is kernels_reg.hpp alone.  Nothing in this file reaches a run-time compiled unit (reg_jit.hpp), and the
// names of the precompiled code objects do not depend on it: editing a launcher or a rule here rebuilds no kernel.
#pragma once

// The stock codes, ONCE: X(id, K, R, G0, G1, G2, G3).  The RegSpec of an id, reg_code_init's lookup, the per-id launchers and
// their dispatch all come from this list; a new code is one line here plus its id in the Makefile's REG_IDS.
#define VIT_REG_STOCK_CODES(X)                                                        \
    X(0, 7, 2, 109, 79, 0, 0)         /* Voyager          (common_codes.h:23) */      \
    X(1, 7, 3, 91, 117, 121, 0)       /* LTE              (:24) */                    \
    X(2, 7, 4, 109, 79, 83, 109)      /* DAB Radio        (:25) */                    \
    X(3, 9, 2, 491, 369, 0, 0)        /* CDMA IS-95A      (:26) */                    \
    X(4, 9, 4, 501, 441, 331, 315)    /* CDMA 2000        (:27) */                    \
    X(5, 3, 2, 7, 5, 0, 0)            /* Basic K=3        (:21)  all 4 states in one lane */  \
    X(6, 5, 2, 23, 25, 0, 0)          /* Basic K=5        (:22)  all 16 states in one lane */

#ifdef VIT_REG_ID
// a reg_inst.hip unit: K and R of its one code, as the preprocessor sees them (kernels_reg.hpp: VIT_REG_UPDATE_VGPR_CAP)
#ifdef VIT_REG_UPDATE_VGPR_CAP
#error "a reg_inst unit includes reg_plan.hpp before kernels_reg.hpp"
#endif
#define VIT_REG_K_IF_ID(id, K, R, g0, g1, g2, g3) +((id) == VIT_REG_ID ? (K) : 0)
#define VIT_REG_R_IF_ID(id, K, R, g0, g1, g2, g3) +((id) == VIT_REG_ID ? (R) : 0)
#define VIT_REG_TU_K (0 VIT_REG_STOCK_CODES(VIT_REG_K_IF_ID))
#define VIT_REG_TU_R (0 VIT_REG_STOCK_CODES(VIT_REG_R_IF_ID))
#endif

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "kernel_desc.hpp"
#include "kernels_reg.hpp"

namespace vit {

// a run-time compiled instantiation (reg_jit.hpp): the same four kernels for polynomials that are not in the list above
struct RegJitModule {
    hipModule_t module = nullptr;
    hipFunction_t update[2] = {nullptr, nullptr};   // [0] 16-bit, [1] 8-bit metrics/symbols
    hipFunction_t resume[2] = {nullptr, nullptr};
    hipFunction_t chainback = nullptr, export_ = nullptr;
    hipFunction_t chainback_alt = nullptr;         // K = 7, 9: the alternative body (reg_chainback_alt_body)
    kd::Table kernels;                              // kernel descriptors of the module's code object (kernel_desc.hpp)
};

struct RegCode {
    int id = -1;   // an id of the list above; -1 with jit != nullptr for a run-time compiled code
    int K = 0, R = 0;
    int tile = 32; // frames per wavefront
    uint32_t G[6] = {0, 0, 0, 0, 0, 0};
    const RegJitModule* jit = nullptr;
    bool generic = false;   // jit is the GENERIC code object of (K, R): the kernels read G from their arguments (RegSpec::GENERIC)
};

// (K, R) with a generic register-plan kernel: the LDS-ring geometries (K = 7: whole-step fetch, K = 8, 9: per sub-chunk) and, below K = 7,
// the one-lane geometry with the pairs parked in LDS; whole patterns (R <= 4)
inline bool reg_generic_supported(int K, int R) {
    // (K = 6 at an odd rate unrolls an 80- to 240-step block: minutes of hipcc per object; K = 2: one butterfly, nothing to look up)
    return K >= 3 && K <= 9 && R >= 1 && R <= 4 && !(K == 6 && (R & 1));
}

// host mirror of RegSpec's geometry: lane bits, frames per wavefront, decision dwords per step, steps per 16-byte row
constexpr int reg_lane_bits(int K) { return K >= 7 ? 2 : 0; }
constexpr int reg_tile_frames(int K) { return K < 7 ? 128 : 32; }
inline size_t reg_steps_per_row(int K) {
    const size_t nreg = (size_t)1 << (K - 1 - reg_lane_bits(K));
    const size_t dw = nreg >= 16 ? nreg / 16 : 1;
    return 4 / dw;
}
inline size_t reg_groups(const RegCode& rc, size_t L) {
    const size_t S = L + (size_t)rc.K - 1;
    const size_t sps = reg_steps_per_row(rc.K);
    return (S + sps - 1) / sps;
}
inline size_t reg_tiles(const RegCode& rc, size_t frames) { return (frames + (size_t)rc.tile - 1) / (size_t)rc.tile; }
inline size_t reg_workspace_bytes(const RegCode& rc, size_t frames, size_t L) {
    return reg_tiles(rc, frames) * reg_groups(rc, L) * 1024;
}

struct RegStockCode { int id, K, R; uint32_t G[4]; };
#define VIT_REG_ROW(id, K, R, g0, g1, g2, g3) {id, K, R, {g0, g1, g2, g3}},
constexpr RegStockCode REG_STOCK_CODES[] = {VIT_REG_STOCK_CODES(VIT_REG_ROW)};
#undef VIT_REG_ROW

inline bool reg_code_supported(int K, int R) {
    for (const RegStockCode& c : REG_STOCK_CODES)
        if (c.K == K && c.R == R) return true;
    return false;
}

inline bool reg_code_init(RegCode* rc, int K, int R, const uint32_t* G, const DevConfig&) {
    for (const RegStockCode& c : REG_STOCK_CODES) {
        if (c.K != K || c.R != R) continue;
        bool same = true;
        for (int i = 0; i < R; ++i) same = same && (c.G[i] == G[i]);
        if (same) {
            rc->id = c.id; rc->K = K; rc->R = R; rc->tile = reg_tile_frames(K);
            for (int i = 0; i < 4; ++i) rc->G[i] = c.G[i];
            rc->G[4] = rc->G[5] = 0;
            return true;
        }
    }
    return false;
}
// the export kernel of a stock code depends on K alone: every code runs the one of the first code of its K
constexpr int reg_export_id(int K) {
    for (const RegStockCode& c : REG_STOCK_CODES)
        if (c.K == K) return c.id;
    return -1;
}

// The kernels are instantiated one code per translation unit (reg_inst.hip, compiled with -DVIT_REG_ID=<id>) so that the
// heavy unrolled bodies build in parallel; these are the per-code launchers those units define.
template <int ID> struct RegSpecOf;
template <int ID> int reg_launch_update(int shift, const RegUpdateArgs& a, unsigned tiles, hipStream_t st);
template <int ID> int reg_launch_chainback(const RegChainbackArgs& a, unsigned tiles, hipStream_t st, bool coop);
template <int ID> int reg_launch_export(const RegExportArgs& a, unsigned blocks, hipStream_t st);
#define VIT_REG_DECLARE(id, K, R, g0, g1, g2, g3)                                                         \
    template <> struct RegSpecOf<id> { using type = RegSpec<K, R, g0, g1, g2, g3, reg_lane_bits(K)>; };   \
    template <> int reg_launch_update<id>(int, const RegUpdateArgs&, unsigned, hipStream_t);              \
    template <> int reg_launch_chainback<id>(const RegChainbackArgs&, unsigned, hipStream_t, bool);       \
    template <> int reg_launch_export<id>(const RegExportArgs&, unsigned, hipStream_t);
VIT_REG_STOCK_CODES(VIT_REG_DECLARE)
#undef VIT_REG_DECLARE
// return VIT_REG_CALL(id) for the id that equals `value`: the caller defines VIT_REG_CALL around its one use of the dispatch
#define VIT_REG_CASE(id, K, R, g0, g1, g2, g3) case id: return VIT_REG_CALL(id);
#define VIT_REG_DISPATCH(value) switch (value) { VIT_REG_STOCK_CODES(VIT_REG_CASE) default: return -1; }

// ---- which kernels can share a SIMD: read from the kernel DESCRIPTORS (kernel_desc.hpp), the numbers the wave launcher uses ----
// (hipFuncGetAttributes().numRegs is the count the code USES; hipcc pads the allocation of kernels whose static LDS limits their
// occupancy -- round 3's K = 9 chainback used 22 registers and allocated 264)
enum RegKernelKind { REG_KERNEL_UPDATE = 0, REG_KERNEL_CHAINBACK = 1, REG_KERNEL_CHAINBACK_ALT = 2, REG_KERNEL_RESUME = 3 };
inline bool reg_kernel_resources(const RegCode& rc, int shift, int kind, kd::KernelResources* out, unsigned* dyn_lds_bytes = nullptr) {
    if (dyn_lds_bytes) *dyn_lds_bytes = kind == REG_KERNEL_CHAINBACK ? reg_chainback_dyn_lds_bytes(rc.K, rc.R, false)
                                      : kind == REG_KERNEL_CHAINBACK_ALT ? reg_chainback_dyn_lds_bytes(rc.K, rc.R, true) : 0u;
    const kd::KernelResources* r = nullptr;
    if (rc.jit) {
        const char* name = kind == REG_KERNEL_UPDATE ? (shift ? "vit_jit_update_8" : "vit_jit_update_16")
                         : kind == REG_KERNEL_RESUME ? (shift ? "vit_jit_resume_8" : "vit_jit_resume_16")
                         : kind == REG_KERNEL_CHAINBACK ? "vit_jit_chainback" : "vit_jit_chainback_alt";
        for (const auto& e : rc.jit->kernels)
            if (e.first == name) r = &e.second;
    } else {
        // Itanium mangling of vit::<kernel><RegSpec<K, R, G0, G1, G2, G3, LANE_BITS, G4, G5>[, SHIFT]>(Args)
        char spec[128], tail[48];
        snprintf(spec, sizeof(spec), "7RegSpecILi%dELi%dELj%uELj%uELj%uELj%uELi%dELj%uELj%uEEE", rc.K, rc.R, rc.G[0], rc.G[1], rc.G[2], rc.G[3],
                 reg_lane_bits(rc.K), rc.G[4], rc.G[5]);
        snprintf(tail, sizeof(tail), "ELi%dEEEvNS_13RegUpdateArgsE", shift ? 8 : 0);
        std::vector<std::string> frag;
        if (kind == REG_KERNEL_UPDATE) frag = {"17reg_update_kernelI", spec, tail};
        else if (kind == REG_KERNEL_RESUME) frag = {"17reg_resume_kernelI", spec, tail};
        else if (kind == REG_KERNEL_CHAINBACK) frag = {"20reg_chainback_kernelI", spec};
        else frag = {"24reg_chainback_alt_kernelI", spec};
        r = kd::find(kd::own_library(), frag);
    }
    if (!r) return false;
    *out = *r;
    return true;
}

constexpr unsigned SIMD_VGPRS = 512, CU_LDS_BYTES = 160 * 1024;
// can `n_update` update waves and one chainback wave of this code share a SIMD: registers (the descriptors' allocations), and per
// CU the LDS of 4 n_update update waves plus two chainback workgroups (a 65536-frame batch is 512 of them on 256 CUs)?  When they
// cannot (K = 9, R = 4: one update wave allocates 360 registers), the chainback of a batch only runs in the gaps between update
// kernels, and the pipeline does better feeding the SIMDs half-size sub-batches from two streams.  Descriptors that cannot be
// read (the library file moved away under the process) answer "no": the conservative schedule.
inline bool reg_chainback_fits_beside_updates(const RegCode& rc, int shift, int n_update, bool alt_chainback = false) {
    kd::KernelResources u, c;
    unsigned dyn = 0;
    if (!reg_kernel_resources(rc, shift, REG_KERNEL_UPDATE, &u) ||
        !reg_kernel_resources(rc, shift, alt_chainback ? REG_KERNEL_CHAINBACK_ALT : REG_KERNEL_CHAINBACK, &c, &dyn))
        return false;
    if ((unsigned)n_update * u.vgpr_alloc + c.vgpr_alloc > SIMD_VGPRS) return false;
    return 4u * (unsigned)n_update * u.lds_static_bytes + 2u * (c.lds_static_bytes + dyn) <= CU_LDS_BYTES;
}

inline int reg_jit_launch(hipFunction_t fn, const void* args, size_t args_bytes, unsigned grid, unsigned block, hipStream_t st,
                          unsigned dyn_lds_bytes = 0) {
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<void*>(args), HIP_LAUNCH_PARAM_BUFFER_SIZE, &args_bytes,
                      HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, dyn_lds_bytes, st, nullptr, config) == hipSuccess ? 0 : -1;
}

// steps [first_step, first_step + n_steps) of every frame.  d_metrics_in == null: reset(start_state) (first_step must be 0);
// else resume from those metrics.  sym_stride: soft_t elements between the chunks of consecutive frames.
inline int reg_update(const RegCode& rc, const DevConfig& cfg, int shift, const void* d_symbols, size_t sym_stride, size_t frames,
                      size_t first_step, size_t n_steps, size_t L, void* d_ws, const void* d_metrics_in, void* d_metrics,
                      uint64_t* d_renorm, const uint32_t* d_start, hipStream_t st) {
    if (frames == 0 || n_steps == 0) return 0;
    RegUpdateArgs a{};
    a.symbols = (const uint8_t*)d_symbols;
    a.sym_frame_stride_bytes = sym_stride * (shift ? 1 : 2);
    // per-lane 32-bit buffer offsets; a resumed call's look-ahead may form slightly negative offsets (see reg_update_body):
    // they must stay distinguishable from valid ones (sign bit) and out of the descriptor's range
    if (a.sym_frame_stride_bytes * (size_t)rc.tile + 65536 >= (d_metrics_in ? 0x7FFF0000ull : 0xFFFF0000ull)) return -2;
    // the last frame's chunk ends n_steps into its stride
    a.sym_total_bytes = (frames - 1) * a.sym_frame_stride_bytes + n_steps * (size_t)rc.R * (shift ? 1 : 2);
    a.ws = (uint4*)d_ws;
    a.ws_tile_stride = reg_groups(rc, L) * 64;
    a.metrics_out = d_metrics;
    a.renorm_sum = d_renorm;
    a.start_state = d_start;
    a.metrics_in = d_metrics_in;
    a.frames = (u32)frames;
    a.t_begin = (u32)first_step;
    a.t_end = (u32)(first_step + n_steps);
    a.cfg = cfg;
    for (int i = 0; i < 6; ++i) a.gen_G[i] = rc.G[i];
#ifdef VIT_HIP_CLOCK_STAMPS
    a.stamps = g_clock_stamps;
#endif
    const unsigned tiles = (unsigned)reg_tiles(rc, frames);
    if (rc.jit) return reg_jit_launch((d_metrics_in ? rc.jit->resume : rc.jit->update)[shift ? 1 : 0], &a, sizeof(a), tiles, 64, st);
#define VIT_REG_CALL(ID) reg_launch_update<ID>(shift, a, tiles, st)
    VIT_REG_DISPATCH(rc.id)
#undef VIT_REG_CALL
}

// `prefer_alt`: launch the code's OTHER chainback kernel (K = 7: the LDS-ring body, 32 registers -- what the pipeline asks for
// when the chainback shares SIMDs with update waves; K = 9: the cooperative body): vit_hip_chainback_batch_ex picks it.
inline int reg_chainback(const RegCode& rc, const void* d_ws, size_t frames, size_t L, uint8_t* d_out, const uint32_t* d_end,
                         hipStream_t st, unsigned wave_priority = 0, bool prefer_alt = false) {
    if (frames == 0 || L == 0) return 0;
    RegChainbackArgs a{};
    a.ws = (const uint4*)d_ws;
    a.ws_tile_stride = reg_groups(rc, L) * 64;
    a.out = d_out;
    a.end_state = d_end;
    a.frames = (u32)frames;
    a.L = (u32)L;
    a.wave_priority = wave_priority;
    const unsigned tiles = (unsigned)reg_tiles(rc, frames);
    // K = 7, 9: the other chainback kernel of the code (reg_chainback_alt_body)
    bool coop = prefer_alt && (rc.K == 9 || rc.K == 7);
#ifdef VIT_HIP_EXPERIMENTS
    if (const char* e = getenv("VIT_HIP_CHAINBACK_ALT")) coop = (rc.K == 9 || rc.K == 7) && *e == '1';   // A/B builds only
#endif
    if (rc.jit) {
        if (coop && rc.jit->chainback_alt)
            return reg_jit_launch(rc.jit->chainback_alt, &a, sizeof(a), rc.K == 9 ? tiles : (unsigned)((frames + 127) / 128), 64, st,
                                  reg_chainback_dyn_lds_bytes(rc.K, rc.R, true));
        const unsigned fpb = reg_chainback_frames_per_block(rc.K);
        return reg_jit_launch(rc.jit->chainback, &a, sizeof(a), (unsigned)((frames + fpb - 1) / fpb), 64, st,
                              reg_chainback_dyn_lds_bytes(rc.K, rc.R, false));
    }
#define VIT_REG_CALL(ID) reg_launch_chainback<ID>(a, tiles, st, coop)
    VIT_REG_DISPATCH(rc.id)
#undef VIT_REG_CALL
}

inline int reg_export(const RegCode& rc, const void* d_ws, size_t frames, size_t n_steps, size_t L, uint64_t* d_out,
                      hipStream_t st) {
    if (frames == 0 || n_steps == 0) return 0;
    RegExportArgs a{};
    a.ws32 = (const u32*)d_ws;
    a.ws_tile_stride = reg_groups(rc, L) * 64;
    a.out = d_out;
    a.frames = (u32)frames;
    a.n_steps = (u32)n_steps;
    const size_t W = rc.K >= 7 ? (size_t)1 << (rc.K - 7) : 1;
    const size_t total = frames * n_steps * W;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (rc.jit) return reg_jit_launch(rc.jit->export_, &a, sizeof(a), blocks, 256, st);
#define VIT_REG_CALL(ID) reg_launch_export<ID>(a, blocks, st)
    VIT_REG_DISPATCH(reg_export_id(rc.K))
#undef VIT_REG_CALL
}

}  // namespace vit
